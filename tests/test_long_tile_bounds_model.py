"""The bounds of the long-block column kernels' tile I/O (long_block_range,
long_tile_bounds, long_tile_class, long_tile_next_straddling and
long_point_valid of csrc/conv_long_kernels.hpp), restated here line for line
and checked against brute force over every element of every instruction.

A (k_long_cols_fwd) loads and C (k_long_cols_inv) stores a tile of 16 columns
with 32 instructions of 16 rows x 16 columns each.  An instruction classified
inside runs with no per-lane test, one classified outside is not issued, the
rest test each lane with long_point_valid.  So the kernels touch exactly the
valid elements when

    inside     => every element of the instruction is in range,
    outside    => none is,
    straddling => the per-lane test equals "in range" element by element,

which is what is asserted, for A against the signal [0, n) and for C against
the block's share [j hop, min(out_len, (j + 1) hop)) of the output; the range
itself is the 64-bit one of the parent kernels (origin + e in [lo, hi)), not
the header's 32-bit form.  The spans of an item's instructions are disjoint,
so each end of the range can make one instruction straddle: at most two per
item, also asserted, together with "straddling => not every element in range"
(the per-lane path is not taken where the plain one would do) and that C's
walk over the straddling instructions visits exactly those.

Sweep: K over the sizes that put skip = K - 1 on and off instruction
boundaries; the signal end and the output end placed mid-instruction, on a
column-0 / row-multiple-of-16 boundary and one element either side of it, and
in the first and last instruction of an item, in block 0, 1 and 3; blocks 0, 1,
the one holding the end and the last; every tile whose columns hold a
boundary, its neighbours, and the first and last tile.  The H build (A with
hop 0 over [0, K)) and empty ranges are swept too.
"""
import numpy as np
import pytest

N1, N2, W = 512, 4096, 16          # kLongN1, kLongN2, kLongW
N = N1 * N2
ROWS = 256 // W                    # kLongTileRows
STEP_LOG2 = 16                     # kLongTileStepLog2
STEP = ROWS * N2                   # kLongTileStep
SPAN = (ROWS - 1) * N2 + W - 1     # kLongTileSpan
NI = N1 // ROWS                    # instructions per item
TILES = N2 // W
INSIDE, OUTSIDE, STRADDLE = 0, 1, 2
assert STEP == 1 << STEP_LOG2 and STEP > SPAN

KS = [1, 17, 4097, 65536, 65537, 100003, 131072, N // 4]


# ------------------------------------------------- the header, restated
def block_range(origin, lo, hi):
    a, b = lo - origin, hi - origin
    l = 0 if a < 0 else N if a > N else a
    h = 0 if b < 0 else N if b > N else b
    return (l, h) if h > l else (0, 0)


def point_valid(e, r):
    """(unsigned)(e - r.lo) < (unsigned)(r.hi - r.lo), on arrays of e."""
    return ((e - r[0]) & 0xFFFFFFFF) < ((r[1] - r[0]) & 0xFFFFFFFF)


def tile_bounds(tile, r):
    t = tile * W
    in_first = (r[0] - t + STEP - 1) >> STEP_LOG2       # Python's >> is a floor too
    in_last = (r[1] - 1 - SPAN - t) >> STEP_LOG2
    any_first = (r[0] - SPAN - t + STEP - 1) >> STEP_LOG2
    any_last = (r[1] - 1 - t) >> STEP_LOG2
    in_count, any_count = in_last - in_first + 1, any_last - any_first + 1
    return in_first, max(in_count, 0), any_first, max(any_count, 0)


def _u32_less(a, b):
    return (a & 0xFFFFFFFF) < (b & 0xFFFFFFFF)


def tile_class(i, b):
    if _u32_less(i - b[0], b[1]):
        return INSIDE
    if _u32_less(i - b[2], b[3]):
        return STRADDLE
    return OUTSIDE


def next_straddling(i, b):
    i += 1
    return i + b[1] if b[1] > 0 and i == b[0] else i


def tile_first(tile, i):
    return tile * W + i * STEP


# ------------------------------------------------- brute force
_ELEM = (N2 * np.arange(ROWS, dtype=np.int64)[:, None] + np.arange(W, dtype=np.int64)[None, :]).ravel()


def _pos(i, r, t, c):
    return i * STEP + r * N2 + t * W + c


# in-block positions of a range end: the element there is the first one out
END_POSITIONS = [
    _pos(5, 7, 100, 5),                                      # mid-instruction
    _pos(16, 0, 0, 0) - 1, _pos(16, 0, 0, 0), _pos(16, 0, 0, 0) + 1,   # instruction boundary of tile 0
    _pos(9, 0, 77, 0) - 1, _pos(9, 0, 77, 0), _pos(9, 0, 77, 0) + 1,   # of a middle tile
    _pos(0, 3, 17, 0), _pos(0, 0, 0, 1),                     # first instruction
    _pos(31, 15, 255, 15), _pos(31, 0, 254, 15), N,          # last instruction; the whole block in range
]


def _tiles_for(boundaries, origin):
    out = {0, TILES - 1}
    for b in boundaries:
        t = ((b - origin) % N2) // W
        out.update(u for u in (t - 1, t, t + 1) if 0 <= u < TILES)
    return sorted(out)


def _check_item(origin, lo, hi, tiles, what):
    """Every instruction of the items `tiles` of one block against brute force
    on the 64-bit definition: element origin + e is valid iff lo <= it < hi."""
    rng = block_range(origin, lo, hi)
    assert 0 <= rng[0] <= rng[1] <= N
    for tile in tiles:
        tb = tile_bounds(tile, rng)
        straddling = []
        for i in range(NI):
            e = tile_first(tile, i) + _ELEM
            g = origin + e
            ok = (g >= lo) & (g < hi)
            cls = tile_class(i, tb)
            where = (what, origin, lo, hi, tile, i)
            if cls == INSIDE:
                assert ok.all(), where
            elif cls == OUTSIDE:
                assert not ok.any(), where
            else:
                assert not ok.all(), where
                assert np.array_equal(point_valid(e, rng), ok), where
                straddling.append(i)
        assert len(straddling) <= 2, (what, origin, lo, hi, tile, straddling)
        walk, i = [], next_straddling(tb[2] - 1, tb)
        while i < tb[2] + tb[3]:
            walk.append(i)
            i = next_straddling(i, tb)
        assert walk == straddling, (what, origin, lo, hi, tile, walk, straddling)
        assert all(0 <= i < NI for i in walk)


def _blocks_to_check(blocks, jt):
    return sorted({j for j in (0, 1, jt, blocks - 1) if 0 <= j < blocks})


@pytest.mark.parametrize("K", KS)
def test_forward_loads(K):
    """A: block j reads x[-(K-1) + j hop + e], valid in [0, n)."""
    hop = N - K + 1
    for jt in (0, 1, 3):
        for p in END_POSITIONS:
            n = -(K - 1) + jt * hop + p
            if n < 1:
                continue
            blocks = -(-(n + K - 1) // hop)
            for j in _blocks_to_check(blocks, jt):
                origin = -(K - 1) + j * hop
                _check_item(origin, 0, n, _tiles_for((0, n), origin), f"A K={K} n={n} j={j}")


@pytest.mark.parametrize("K", KS)
def test_inverse_stores(K):
    """C: point e >= skip of block j goes to y[j hop + e - skip], below out_len."""
    hop, skip = N - K + 1, K - 1
    for jt in (0, 1, 3):
        for p in END_POSITIONS:
            out_len = jt * hop - skip + p
            if out_len <= jt * hop:
                continue  # the end has to lie in block jt
            blocks = -(-out_len // hop)
            for j in _blocks_to_check(blocks, jt):
                origin, lo = j * hop - skip, j * hop
                hi = min(out_len, lo + hop)
                assert hi > lo
                _check_item(origin, lo, hi, _tiles_for((lo, hi), origin), f"C K={K} out_len={out_len} j={j}")


@pytest.mark.parametrize("K", KS)
def test_h_build(K):
    """A building H: one block at origin 0 over the K taps; instructions that
    begin at or after tap K are outside."""
    _check_item(0, 0, K, _tiles_for((0, K), 0), f"H K={K}")
    tile = TILES // 2
    tb = tile_bounds(tile, block_range(0, 0, K))
    for i in range(NI):
        if tile_first(tile, i) >= K:
            assert tile_class(i, tb) == OUTSIDE


def test_empty_and_far_ranges():
    """No signal, a block wholly before or after the range, and a range wider
    than the block: nothing valid, or everything."""
    for origin, lo, hi in [(0, 0, 0), (-5, 0, 0), (100, 0, 50), (-3 * N, 0, 10), (7, 0, -4)]:
        assert block_range(origin, lo, hi) == (0, 0)
        _check_item(origin, lo, hi, [0, 1, TILES - 1], "empty")
    for tile in (0, 77, TILES - 1):
        tb = tile_bounds(tile, block_range(12345, -10 * N, 10 * N))
        assert all(tile_class(i, tb) == INSIDE for i in range(NI))
    _check_item(12345, -10 * N, 10 * N, [0, TILES - 1], "all")


def test_bench_shape_counts():
    """Stereo 2^24 through K = 131072, nine blocks: blocks 1 .. 7 of A are
    wholly inside; C never stores instruction 0, and its instruction 1 only in
    the last tile."""
    K, n = 131072, 1 << 24
    hop, skip = N - K + 1, K - 1
    out_len = n + K - 1
    blocks = -(-out_len // hop)
    assert blocks == 9
    for j in range(1, 8):
        rng = block_range(-(K - 1) + j * hop, 0, n)
        for tile in (0, 100, TILES - 1):
            tb = tile_bounds(tile, rng)
            assert all(tile_class(i, tb) == INSIDE for i in range(NI))
    for j in (0, 4, 8):
        lo = j * hop
        rng = block_range(lo - skip, lo, min(out_len, lo + hop))
        for tile in range(TILES):
            tb = tile_bounds(tile, rng)
            assert tile_class(0, tb) == OUTSIDE
            assert tile_class(1, tb) == (STRADDLE if tile == TILES - 1 else OUTSIDE)
