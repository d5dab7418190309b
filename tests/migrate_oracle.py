"""NumPy model of a particle's way between ranks (include/rbpf_hip.h: rbpf_gather_pack_meta, rbpf_meta_from_raw,
rbpf_pack_particles_raw, rbpf_apply_resample_local, rbpf_unpack_particles), written from the documented wire format alone.

A particle is its state (pose, 3x3 covariance, weight), its tiles (centre in metres -> int8 cells [dim, dim], indexed [x][y])
and the written box of every tile ((x0, x1, y0, y1) inclusive, None: held but nothing written).

  records   [n][L*L][5]      per departing particle and lattice position pos = (lx + R) * L + (ly + R):
                             (held, x0, x1, y0, y1); an unwritten tile has the empty box (INT_MAX, -1, INT_MAX, -1), a position
                             that is not held has zeros.  (The device's first field is a pool index: >= 0 iff held.)
  meta      [n][2 + 6*L*L]   tile count, payload bytes / 16, then per position (has, x0, x1, y0, y1, offset / 16), the offset
                             counted from the start of the particle's payload; an unwritten tile is (1, 0, -1, 0, -1, offset).
  payload                    per particle a 128-byte state block - 13 doubles x, y, theta, cov[0..8], weight, 24 bytes undefined -
                             then per written tile, in position order: rows x0..x1 of the columns [ya, yb) as int8, ya = y0 & ~15,
                             yb = min((y1 | 15) + 1, dim), then (x1 - x0 + 1) * ow occupancy words (uint32, little endian; bit
                             y & 31 of word y >> 5 set iff the cell's value is above occupied_threshold / quantum), the whole
                             padded to a multiple of 16 bytes (padding undefined).  An unwritten tile takes no bytes.

arrive() is what the receiving rank holds after rbpf_apply_resample_local and rbpf_unpack_particles."""
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from tests import resample_oracle as R

INT_MAX = 2 ** 31 - 1
STATE_BYTES = 128
TILE_LEN = 40.0


class State(NamedTuple):
    poses: np.ndarray                      # [P, 3]
    covs: np.ndarray                       # [P, 3, 3]
    weights: np.ndarray                    # [P]
    maps: List[R.Tiles]
    boxes: List[Optional[Dict[R.Centre, R.Box]]]   # None for a particle: the boxes of its tiles' non-zero cells

    @property
    def tiles_in_use(self):
        return sum(len(m) for m in self.maps)


def position(centre, L, Rr, tile_len=TILE_LEN):
    lx, ly = int(round(centre[0] / tile_len)), int(round(centre[1] / tile_len))
    assert -Rr <= lx <= Rr and -Rr <= ly <= Rr
    return (lx + Rr) * L + (ly + Rr)


def centre_of(pos, L, Rr, tile_len=TILE_LEN):
    return (float((pos // L - Rr) * tile_len), float((pos % L - Rr) * tile_len))


def box_of(maps, boxes, p, c) -> R.Box:
    return R.written_box(maps[p][c]) if boxes is None or boxes[p] is None else boxes[p][c]


def round16(n):
    return (int(n) + 15) // 16 * 16


def columns(y0, y1, dim):
    return y0 // 16 * 16, min((y1 // 16 + 1) * 16, dim)


def raw_records(maps, boxes, leaving, L, Rr, tile_len=TILE_LEN):
    out = np.zeros((len(leaving), L * L, 5), dtype=np.int64)
    for i, p in enumerate(leaving):
        for c in maps[p]:
            b = box_of(maps, boxes, p, c)
            out[i, position(c, L, Rr, tile_len)] = (1, INT_MAX, -1, INT_MAX, -1) if b is None else (1,) + tuple(b)
    return out


def meta_rows(raw, dim, ow) -> Tuple[np.ndarray, int]:
    raw = np.asarray(raw)
    n, LL = raw.shape[0], raw.shape[1]
    rows = np.zeros((n, 2 + 6 * LL), dtype=np.int64)
    total = 0
    for i in range(n):
        off = STATE_BYTES
        for pos in range(LL):
            held, x0, x1, y0, y1 = (int(v) for v in raw[i, pos])
            if not held:
                continue
            rows[i, 0] += 1
            if x0 > x1 or y0 > y1:
                rows[i, 2 + 6 * pos:8 + 6 * pos] = (1, 0, -1, 0, -1, off // 16)
                continue
            rows[i, 2 + 6 * pos:8 + 6 * pos] = (1, x0, x1, y0, y1, off // 16)
            ya, yb = columns(y0, y1, dim)
            off += round16((x1 - x0 + 1) * (yb - ya) + 4 * (x1 - x0 + 1) * ow)
        rows[i, 1] = off // 16
        total += off
    return rows, total


def closed_form_bytes(raw, dim, ow):
    raw = np.asarray(raw)
    total = STATE_BYTES * raw.shape[0]
    for held, x0, x1, y0, y1 in raw.reshape(-1, 5):
        if held and x0 <= x1 and y0 <= y1:
            ya, yb = columns(int(y0), int(y1), dim)
            total += round16(int(x1 - x0 + 1) * (yb - ya) + 4 * int(x1 - x0 + 1) * ow)
    return total


def occupancy_words(cells, ow, thr):
    """uint32 [dim, ow] of a tile: bit y & 31 of word y >> 5 of row x."""
    dim = cells.shape[0]
    occ = np.zeros((dim, ow * 32), dtype=np.uint8)
    occ[:, :dim] = cells.astype(np.int64) > thr
    return np.packbits(occ, axis=1, bitorder="little").view("<u4").astype(np.uint32)


def threshold(quantum, occupied_threshold):
    return int(np.floor(float(occupied_threshold) / float(quantum) + 1e-9))


def payload(state: State, leaving, dim, ow, thr, L, Rr, tile_len=TILE_LEN):
    """(uint8 bytes, bool mask of the defined bytes, meta rows) of the particles `leaving`, in that order."""
    raw = raw_records(state.maps, state.boxes, leaving, L, Rr, tile_len)
    meta, total = meta_rows(raw, dim, ow)
    buf, known = np.zeros(total, dtype=np.uint8), np.zeros(total, dtype=bool)
    start = 0
    for i, p in enumerate(leaving):
        block = np.concatenate([state.poses[p], np.asarray(state.covs[p]).reshape(9), [state.weights[p]]]).astype("<f8")
        buf[start:start + 104] = block.view(np.uint8)
        known[start:start + 104] = True
        for pos in range(L * L):
            has, x0, x1, y0, y1, off16 = (int(v) for v in meta[i, 2 + 6 * pos:8 + 6 * pos])
            if not has or x0 > x1:
                continue
            cells = state.maps[p][centre_of(pos, L, Rr, tile_len)]
            ya, yb = columns(y0, y1, dim)
            part = np.ascontiguousarray(cells[x0:x1 + 1, ya:yb]).view(np.uint8).reshape(-1)
            words = np.ascontiguousarray(occupancy_words(cells, ow, thr)[x0:x1 + 1]).astype("<u4").view(np.uint8).reshape(-1)
            at = start + 16 * off16
            buf[at:at + len(part)] = part
            buf[at + len(part):at + len(part) + len(words)] = words
            known[at:at + len(part) + len(words)] = True
        start += 16 * int(meta[i, 1])
    assert start == total
    return buf, known, meta


def unpack(buf, meta, dim, ow, L, Rr, tile_len=TILE_LEN):
    """The reverse of payload(): per particle (13 doubles, tiles, boxes, occupancy words [dim, ow] per tile)."""
    out, start = [], 0
    for row in np.asarray(meta):
        state = np.frombuffer(np.ascontiguousarray(buf[start:start + 104]).tobytes(), dtype="<f8")
        tiles, boxes, words = {}, {}, {}
        for pos in range(L * L):
            has, x0, x1, y0, y1, off16 = (int(v) for v in row[2 + 6 * pos:8 + 6 * pos])
            if not has:
                continue
            c = centre_of(pos, L, Rr, tile_len)
            tiles[c], words[c], boxes[c] = np.zeros((dim, dim), np.int8), np.zeros((dim, ow), np.uint32), None
            if x0 > x1:
                continue
            ya, yb = columns(y0, y1, dim)
            rows, at = x1 - x0 + 1, start + 16 * off16
            n = rows * (yb - ya)
            tiles[c][x0:x1 + 1, ya:yb] = np.ascontiguousarray(buf[at:at + n]).view(np.int8).reshape(rows, yb - ya)
            words[c][x0:x1 + 1] = np.frombuffer(np.ascontiguousarray(buf[at + n:at + n + 4 * rows * ow]).tobytes(),
                                                dtype="<u4").reshape(rows, ow)
            boxes[c] = (x0, x1, y0, y1)
        assert len(tiles) == row[0]
        out.append((state, tiles, boxes, words))
        start += 16 * int(row[1])
    assert start == len(buf)
    return out


def arrive(recv: State, new_src, arrivals: Sequence[int], send: Optional[State], leaving: Sequence[int]) -> State:
    """The receiver after rbpf_apply_resample_local(new_src) and rbpf_unpack_particles(arrivals): survivor j continues
    recv's particle new_src[j]; arrival arrivals[k] is exactly send's particle leaving[k]; every weight restarts at 1.0."""
    new_src = np.asarray(new_src, dtype=np.int64)
    P = len(new_src)
    arrivals = [int(j) for j in arrivals]
    assert len(arrivals) == len(leaving) and arrivals == [int(j) for j in np.nonzero(new_src < 0)[0]]
    stay = new_src[new_src >= 0]
    assert len(stay) + len(arrivals) == P and np.all(new_src[:len(stay)] >= 0)             # the arrivals come last
    idx = np.concatenate([stay, np.full(len(arrivals), stay[-1] if len(stay) else 0)])     # placeholders, overwritten below
    m = R.move(recv.poses, recv.covs, recv.weights, recv.maps, idx, True)
    poses, covs, maps = m.poses, m.covs, list(m.maps)
    boxes = [recv.boxes[i] for i in idx]
    for j, p in zip(arrivals, leaving):
        poses[j], covs[j], maps[j], boxes[j] = send.poses[p], send.covs[p], send.maps[p], send.boxes[p]
    return State(poses, covs, np.ones(P), maps, boxes)


def extents(state: State, dim, tile_len=TILE_LEN):
    return [R.extent(m, dim, tile_len, b) for m, b in zip(state.maps, state.boxes)]


def whole_lattice(tile_len=TILE_LEN):
    """Written boxes of a particle that holds all 49 tiles (dim 400), each box different."""
    centres = [(tile_len * a, tile_len * b) for a in range(-3, 4) for b in range(-3, 4)]
    return {c: (7 * k, 7 * k + 2 + k % 3, 390 - 8 * k, 399 - 8 * k + k % 5) for k, c in enumerate(centres)}
