"""The binding's plumbing without a library or a GPU: engine._Outputs (where a call's outputs live and how the call is ordered
against torch's stream) over a bare ParticleEngine and a stub torch that record what happens, and the argument helpers every
query method shares (particle_index, _box4, _scan_batch, _poses_angles, _int8_cells)."""
import ctypes as C
import sys
import types
from types import SimpleNamespace

import numpy as np
import pytest

from thesis_amd import engine as E
from thesis_amd.engine import ParticleEngine

TORCH_STREAM = 0x5000           # the handle of the stub torch's current stream


class StubTensor:
    def __init__(self, shape, dtype, device, address=0x1000):
        self.shape, self.dtype, self.device = tuple(np.atleast_1d(shape)), dtype, device
        self._address = address if int(np.prod(self.shape)) else 0        # an empty tensor has no data pointer

    def data_ptr(self):
        return self._address


def stub_torch(events):
    """A module that looks enough like torch for _Outputs, and writes what is asked of it into `events`."""
    t = types.ModuleType("torch")
    for name in ("int8", "uint8", "int16", "uint16", "int32", "int64", "uint64", "float32", "float64"):
        setattr(t, name, "torch." + name)
    t.device = lambda kind, index: (kind, index)

    def empty(shape, dtype, device):
        events.append(("empty", tuple(np.atleast_1d(shape)), dtype, device))
        return StubTensor(shape, dtype, device)

    def current_stream(device):
        return SimpleNamespace(cuda_stream=TORCH_STREAM, synchronize=lambda: events.append("cur.synchronize"))
    t.empty, t.cuda = empty, SimpleNamespace(current_stream=current_stream)
    return t


class UntouchableTorch(types.ModuleType):
    def __getattr__(self, name):
        raise AssertionError(f"torch.{name} was touched on a numpy-only path")


def bare_engine(events, borrowed=None, weights=None):
    """A ParticleEngine with no library behind it: what _Outputs and particle_index read, and recorders for what they call."""
    e = object.__new__(ParticleEngine)
    e.cfg = SimpleNamespace(device=3)
    e._borrowed_stream, e._stream_ptr = borrowed is not None, borrowed
    e.synchronize = lambda: events.append("engine.synchronize")

    def read_weights():
        events.append("weights")
        return np.asarray(weights, dtype=np.float64)
    e.weights = read_weights
    return e


@pytest.fixture
def events(monkeypatch):
    ev = []
    monkeypatch.setitem(sys.modules, "torch", stub_torch(ev))
    return ev


def run(e, events, device, adopt=None, fail=False):
    out = e._outputs(device)
    if adopt is not None:
        out.adopt(adopt)
    a, b = out.empty((2, 3), "int32"), out.empty(4, np.float64)
    with out:
        events.append("call")
        if fail:
            raise E.RbpfError(7, "refused")
    return a, b


ALLOCATIONS = [("empty", (2, 3), "torch.int32", ("cuda", 3)), ("empty", (4,), "torch.float64", ("cuda", 3))]


def test_device_outputs_on_the_engines_own_stream_wait_on_both_sides(events):
    a, b = run(bare_engine(events), events, True)
    assert events == ALLOCATIONS + ["cur.synchronize", "call", "engine.synchronize"]
    assert isinstance(a, StubTensor) and a.dtype == "torch.int32" and b.shape == (4,)


def test_a_borrowed_stream_that_is_torchs_current_one_waits_for_nothing(events):
    run(bare_engine(events, borrowed=TORCH_STREAM), events, True)
    assert events == ALLOCATIONS + ["call"]


def test_a_borrowed_stream_other_than_torchs_current_one_waits_on_both_sides(events):
    run(bare_engine(events, borrowed=TORCH_STREAM + 8), events, True)
    assert events == ALLOCATIONS + ["cur.synchronize", "call", "engine.synchronize"]


def test_a_failed_call_propagates_and_is_not_waited_for(events):
    with pytest.raises(E.RbpfError, match="refused"):
        run(bare_engine(events), events, True, fail=True)
    assert events == ALLOCATIONS + ["cur.synchronize", "call"]


def test_an_adopted_tensor_orders_a_host_output_call_behind_torch(events):
    t = StubTensor((5, 5), "torch.int8", ("cuda", 3))
    a, b = run(bare_engine(events), events, False, adopt=t)
    assert events == ["cur.synchronize", "call"]
    assert isinstance(a, np.ndarray) and a.dtype == np.int32 and isinstance(b, np.ndarray) and b.dtype == np.float64
    events.clear()
    run(bare_engine(events, borrowed=TORCH_STREAM), events, False, adopt=t)
    assert events == ["call"]


def test_host_outputs_never_touch_torch(events, monkeypatch):
    monkeypatch.setitem(sys.modules, "torch", UntouchableTorch("torch"))
    a, b = run(bare_engine(events), events, False, adopt=np.zeros((5, 5), np.int8))     # a numpy input is held, no more
    assert events == ["call"]
    assert isinstance(a, np.ndarray) and a.dtype == np.int32 and a.shape == (2, 3)
    assert isinstance(b, np.ndarray) and b.dtype == np.float64 and b.shape == (4,)


def test_device_dtype_absent_and_empty_outputs(events):
    e = bare_engine(events)
    dev, host = e._outputs(True), e._outputs(False)
    assert dev.empty((2, 2), "uint16", device_dtype="int16").dtype == "torch.int16"
    assert host.empty((2, 2), "uint16", device_dtype="int16").dtype == np.uint16
    assert dev.empty((2, 4), "uint64", device_dtype="int64").dtype == "torch.int64"
    assert host.empty((2, 4), "uint64", device_dtype="int64").dtype == np.uint64
    assert dev.ptr(None) is None and host.ptr(None) is None
    for out in (dev, host):
        full, none = out.empty((2, 2), "int32"), out.empty((0, 7), "int32")
        assert isinstance(out.ptr(full), C.c_void_p) and out.ptr(full).value not in (None, 0, 1)
        assert out.ptr(none).value not in (None, 0)
    assert dev.ptr(dev.empty((0, 7), "int32")).value == 1                 # no address: a dummy the library never follows
    a = host.empty((3,), "float64")
    assert host.ptr(a).value == a.ctypes.data


# ---- the argument helpers ----------------------------------------------------------------------------------------------------------
def test_particle_index():
    ev = []
    e = bare_engine(ev, weights=[0.1, 0.7, 0.7, 0.2])
    assert e._particle(2) == 2 and e._particle(np.int64(3)) == 3 and ev == []
    assert e._particle(None) == -1 and ev == []
    assert e._particle("best") == 1 and ev == ["weights"]                # the first argmax
    with pytest.raises(ValueError) as err:
        e._particle("worst")
    assert str(err.value) == "unknown particle 'worst'" and ev == ["weights"]
    with pytest.raises(TypeError):
        e._particle(None, allow_none=False)                               # what int(None) raises
    assert E.particle_index(SimpleNamespace(weights=lambda: np.array([0.0, 2.0])), "best") == 1   # any object with weights()


def test_box4():
    calls = []

    def default():
        calls.append(1)
        return (1, 4, -2, 3)
    b, shape = E._box4((0, 2, 5, 9), default)
    assert calls == [] and b.dtype == np.int32 and b.tolist() == [0, 2, 5, 9] and shape == (2, 4)
    b, shape = E._box4(None, default)
    assert calls == [1] and b.tolist() == [1, 4, -2, 3] and shape == (3, 5)
    with pytest.raises(ValueError) as err:
        E._box4((0, 2, 5), default)
    assert str(err.value) == "box must be (x0, x1, y0, y1)"
    b, shape = E._box4((4, 1, 0, 6), default)                             # inverted in x: the library's to refuse
    assert b.tolist() == [4, 1, 0, 6] and shape == (0, 6)
    assert E._box4(np.array([0.0, 3.0, 7.0, 2.0]), default)[1] == (3, 0) and calls == [1]


def test_scan_batch_and_poses_angles():
    ps, rg, a = E._scan_batch([1.0, 2.0, 0.5], [4.0, 5.0], [0.0, 0.1])
    assert ps.shape == (1, 3) and rg.shape == (1, 2) and a.shape == (2,)
    assert all(x.dtype == np.float64 and x.flags.c_contiguous for x in (ps, rg, a))
    ps, rg, a = E._scan_batch(np.zeros((4, 3)), np.ones((4, 5), np.float32), np.zeros(5))
    assert ps.shape == (4, 3) and rg.shape == (4, 5) and rg.dtype == np.float64
    for bad in ((np.zeros((4, 3)), np.ones((3, 5)), np.zeros(5)), (np.zeros((4, 3)), np.ones((4, 6)), np.zeros(5)),
                (np.zeros((4, 2)), np.ones((4, 5)), np.zeros(5)), (np.zeros((4, 3)), np.ones((4, 5)), np.zeros((1, 5)))):
        with pytest.raises(ValueError) as err:
            E._scan_batch(*bad)
        assert str(err.value) == "poses must be [N, 3], angles [B] and ranges [N, B]"
    ps, a = E._poses_angles([1.0, 2.0, 0.5], [0.0, 0.1])
    assert ps.shape == (1, 3) and a.shape == (2,)
    for bad in ((np.zeros((4, 2)), np.zeros(5)), (np.zeros((4, 3)), np.zeros((5, 1))), (np.zeros((2, 4, 3)), np.zeros(5))):
        with pytest.raises(ValueError) as err:
            E._poses_angles(*bad)
        assert str(err.value) == "poses must be [N, 3] (or [3]) and angles 1-D"


def test_int8_cells(events):
    e = bare_engine(events)
    cells, shape = e._int8_cells(np.array([[-128, 0, 127], [5, -5, 30]], np.int16), "raster", "[nx][ny]")
    assert cells.dtype == np.int8 and cells.flags.c_contiguous and shape == (2, 3) and cells.tolist() == [[-128, 0, 127], [5, -5, 30]]
    same = np.zeros((3, 2), np.int8)
    assert e._int8_cells(same, "source", "[nsx][nsy]")[0] is same
    assert e._int8_cells(np.zeros((6, 4), np.int8)[::2], "source", "[nsx][nsy]")[0].flags.c_contiguous
    for bad, what, axes, msg in ((np.array([[0, 128]], np.int16), "raster", "[nx][ny]", "raster cells must be int8 lattice values"),
                                 (np.array([[0.0, 1.0]]), "source", "[nsx][nsy]", "source cells must be int8 lattice values"),
                                 (np.zeros((2, 2, 2), np.int8), "reference", "[nx][ny]", "reference cells must be 2-D [nx][ny]"),
                                 (np.zeros(4, np.int8), "source", "[nsx][nsy]", "source cells must be 2-D [nsx][nsy]")):
        with pytest.raises(ValueError) as err:
            e._int8_cells(bad, what, axes)
        assert str(err.value) == msg
    t = StubTensor((4, 5), "torch.int8", ("cuda", 3))
    t.dim, t.contiguous = (lambda: 2), (lambda: t)
    assert e._int8_cells(t, "raster", "[nx][ny]") == (t, (4, 5))
    t.device = ("cuda", 0)
    with pytest.raises(ValueError) as err:
        e._int8_cells(t, "reference", "[nx][ny]")
    assert str(err.value) == "a tensor reference must be 2-D int8 on ('cuda', 3)"
