"""algodsp.resample on the GPU against the restated reference (resample_ref):
every comparison is bit equality of the float64 images, no tolerance anywhere.
Shapes are the smallest that reach each kernel path: every combination of
where the coefficient table and the input window live, one tile, the tile's
edges, several tiles per workgroup, and calls that produce no output.  Device
buffers handed to the library are guarded placements (layout_lib) the test
owns whole."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import layout_lib as LL
import resample_ref as RR
from algodsp import _lib, irlib, resample as R
from algodsp._lib import lib, ptr

pytestmark = pytest.mark.gpu
DEV = "cuda"
CH = 3
ALL_SHAPES = RR.SHAPES + RR.MORE_SHAPES


def sync():
    import torch

    torch.cuda.synchronize()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


@functools.lru_cache(maxsize=None)
def taps_for(up, down, T, kind):
    """The designer's prototype, or random asymmetric taps of the same length."""
    g = math.gcd(up, down)
    if kind == "designed":
        t = R.design_polyphase_fir(up // g, down // g, T, 0.92, 7.5)
    else:
        t = RR.random_taps(up // g, T, 1000 * up + down + T)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def signal(n, seed=0):
    x = RR.random_input(CH, n, 0xA5 + n + seed)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def want(up, down, T, kind, n, chunks=None):
    """Reference output of signal(n), computed once per case and shared."""
    y, lens = RR.resample(up, down, taps_for(up, down, T, kind), signal(n), chunks=chunks)
    y.setflags(write=False)
    return y, tuple(lens)


def make(up, down, T, kind, channels=CH):
    return R.NewRational(up, down, channels=channels, taps=taps_for(up, down, T, kind))


def tile_edge_inputs(up, down, tile):
    """Input lengths whose output length is one less than, equal to and one
    more than a tile (or, where the ratio steps over one of them, the nearest
    on either side)."""
    ns = set()
    for t in (tile - 1, tile, tile + 1):
        ns.update({(t * down) // up, -((-t * down) // up)})
    return sorted(n for n in ns if n >= 1)


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize("kind", ["designed", "random"])
@pytest.mark.parametrize("up,down,T", ALL_SHAPES)
def test_process_matches_reference(gpu, up, down, T, kind):
    """One call over 3 channels at n_in = 1500 and 4099 and around one tile,
    a fresh handle each."""
    r = make(up, down, T, kind)
    info = r.kernel_info()
    r.close()
    tile, tpw = info["tile"], info["tiles_per_workgroup"]
    g = math.gcd(up, down)
    sizes = list(RR.N_IN) + tile_edge_inputs(up // g, down // g, tile)
    if tpw > 1:  # a workgroup walks several tiles: two full workgroups and part of a third
        sizes.append(-((-(2 * tpw + 3) * tile * down) // up) + 5)
    seen = set()
    for n in sizes:
        w, _ = want(up, down, T, kind, n)
        r = make(up, down, T, kind)
        assert r.PredictOutputLen(n) == w.shape[1]
        y = r.Process(signal(n))
        r.close()
        assert same(y, w), (up, down, T, kind, n)
        seen.add(w.shape[1])
    assert min(seen) < tile < max(seen)
    assert tpw == 1 or max(seen) > 2 * tpw * tile
    if up <= down:  # the output length grows by at most one per input sample: every length is reachable
        assert {tile - 1, tile, tile + 1} <= seen


def test_kernel_paths_are_all_reached(gpu):
    """The shapes above cover both table paths and both window paths, with and
    without a shared phase (up <= 256)."""
    combos, walks = set(), set()
    for up, down, T in ALL_SHAPES:
        r = make(up, down, T, "random", channels=1)
        k = r.kernel_info()
        r.close()
        combos.add((up <= 256, k["table_in_lds"], k["window_in_lds"]))
        if k["tiles_per_workgroup"] > 1:
            walks.add((up <= 256, k["window_in_lds"], k["window_prefetch"]))
        else:
            assert not k["window_prefetch"]
        assert k["lds_bytes"] <= 65536
    assert len(combos) == 8
    # several tiles per workgroup: window loaded ahead (either phase sharing), staged per tile, and not staged
    assert {(True, True, True), (False, True, True), (True, True, False), (False, False, False)} <= walks
    r = make(4097, 4096, 16, "random", channels=1)
    assert not r.kernel_info()["table_in_lds"]
    r.close()


# --------------------------------------------------------------- streaming
def stream(r, x, chunk):
    """x through r in `chunk`-sample calls: the concatenation, the output
    length of every call, and PredictOutputLen called just before each."""
    parts, lens, preds = [], [], []
    for s in range(0, x.shape[1], chunk):
        blk = np.ascontiguousarray(x[:, s:s + chunk])
        preds.append(r.PredictOutputLen(blk.shape[1]))
        y = r.Process(blk)
        parts.append(y)
        lens.append(y.shape[1])
    return np.concatenate(parts, axis=1), lens, preds


@pytest.mark.parametrize("up,down,T", [(160, 147, 32), (1, 6, 16), (5, 3, 64)])
@pytest.mark.parametrize("chunk", [257, 3])
def test_streaming_equals_one_call(gpu, up, down, T, chunk):
    n = 1500
    w, _ = want(up, down, T, "random", n)
    wc, wlens = want(up, down, T, "random", n, chunk)
    assert same(w, wc)  # the reference itself: chunking changes no bit
    r = make(up, down, T, "random")
    y, lens, preds = stream(r, signal(n), chunk)
    r.close()
    assert lens == preds == list(wlens)
    assert same(y, w)
    if (up, down, chunk) == (1, 6, 3):
        assert 0 in lens


@pytest.mark.parametrize("up,down,T", [(160, 147, 32), (1, 6, 16), (5, 3, 64)])
def test_streaming_one_sample_calls(gpu, up, down, T):
    n = 300
    x = signal(1500)[:, :n]
    w, _ = want(up, down, T, "random", 1500)
    r = make(up, down, T, "random")
    y, lens, preds = stream(r, x, 1)
    r.close()
    assert lens == preds
    assert same(y, w[:, :y.shape[1]])
    one = RR.Ref(up, down, taps_for(up, down, T, "random"))
    assert y.shape[1] == len(one.process_vec(x[0]))


def test_mixed_streams(gpu):
    """Calls on the NULL stream, a side stream and the host-buffer path, then
    Reset while a side-stream call is the last one enqueued, then the same
    again: the delay line and the phase are shared by every stream, each call
    waits for the previous call's last operation, so the outputs are one
    sequential resampler's.  5/3 with 64 taps per phase: the 40-sample call is
    shorter than the delay line (63), which is then built from its own tail
    and the input."""
    import torch

    up, down, T, n = 5, 3, 64, 1500
    x = signal(n)[:2].copy()
    w = want(up, down, T, "random", n)[0][:2]  # channels are independent
    cap = w.shape[1]
    r = make(up, down, T, "random", channels=2)
    dx = torch.from_numpy(x).cuda()
    spare = torch.empty((2, 200), dtype=torch.float64, device=DEV)
    side = torch.cuda.Stream()
    for rep in range(2):
        dy = torch.full((2, cap), float("nan"), dtype=torch.float64, device=DEV)
        sync()
        pos = out = 0
        for m, where in [(600, 0), (40, side.cuda_stream), (360, "host"), (500, 0)]:
            if where == "host":
                host_at, host_y = out, r.Process(np.ascontiguousarray(x[:, pos:pos + m]))
                no = host_y.shape[1]
            else:
                no = r.process_device(dx.data_ptr() + 8 * pos, n, m, dy.data_ptr() + 8 * out, cap, cap - out, where)
            pos, out = pos + m, out + no
        sync()
        got = dy.cpu().numpy()
        got[:, host_at:host_at + host_y.shape[1]] = host_y
        assert out == cap and same(got, w), rep
        r.process_device(dx.data_ptr(), n, 100, spare.data_ptr(), 200, 200, side.cuda_stream)
        r.Reset()
    r.close()


def test_zero_output_calls_write_nothing(gpu):
    """1/6 fed 3 samples at a time: the calls that yield no output return
    success, leave a NaN-filled output untouched (host and device form), and
    still take the samples in."""
    up, down, T = 1, 6, 16
    x = signal(1500)
    w, _ = want(up, down, T, "random", 1500)
    L = lib()
    for device_form in (False, True):
        r = make(up, down, T, "random")
        got, zero_calls = [], 0
        for s in range(0, 300, 3):
            blk = np.ascontiguousarray(x[:, s:s + 3])
            n_out = C.c_int64(-1)
            if device_form:
                src = LL.place(blk, LL.L1, DEV)
                dst = LL.empty(CH, 4, LL.L1, DEV)
                sync()
                rc = L.ad_resampler_process_device(r._h, C.c_void_p(src.ptr), src.stride, 3, C.c_void_p(dst.ptr),
                                                   dst.stride, 4, C.byref(n_out), None)
                sync()
                assert rc == _lib.AD_OK
                LL.check_unchanged(src, blk)
                LL.check_guards(dst, untouched=[(n_out.value, 4)])
                y = LL.payload(dst)[:, :n_out.value]
            else:
                out = np.full((CH, 4), np.nan)
                before = bits(out).copy()
                rc = L.ad_resampler_process(r._h, ptr(blk), 3, ptr(out), 4, C.byref(n_out))
                assert rc == _lib.AD_OK
                if n_out.value == 0:
                    assert np.array_equal(bits(out), before)
                y = out.reshape(-1)[:CH * n_out.value].reshape(CH, n_out.value)  # packed at row length n_out
            assert n_out.value in (0, 1)
            zero_calls += n_out.value == 0
            got.append(y.copy())
        r.close()
        y = np.concatenate(got, axis=1)
        assert zero_calls == 50 and y.shape[1] == 50
        assert same(y, w[:, :50])


def test_empty_input_is_a_no_op(gpu):
    r = make(3, 2, 32, "random")
    n_out = C.c_int64(-1)
    assert lib().ad_resampler_process(r._h, None, 0, None, 0, C.byref(n_out)) == _lib.AD_OK
    assert n_out.value == 0
    assert r.PredictOutputLen(0) == 0 and r.PredictOutputLen(-5) == 0
    w, _ = want(3, 2, 32, "random", 1500)
    assert same(r.Process(signal(1500)), w)
    r.close()
    assert R.Resample(np.zeros(0), 3, 2).shape == (0,)


# ------------------------------------------------------- state and errors
def test_reset_reproduces_the_first_output(gpu):
    up, down, T = 160, 147, 32
    w, _ = want(up, down, T, "designed", 1500)
    r = make(up, down, T, "designed")
    assert same(r.Process(signal(1500)), w)
    r.Process(np.ascontiguousarray(signal(4099)[:, :77]))  # leave a phase and a delay line behind
    r.Reset()
    assert same(r.Process(signal(1500)), w)
    r.close()


def test_short_output_fails_and_leaves_the_state(gpu):
    up, down, T = 160, 147, 32
    x = signal(1500)
    first, second = np.ascontiguousarray(x[:, :700]), np.ascontiguousarray(x[:, 700:])
    calm = make(up, down, T, "random")
    y0, y1 = calm.Process(first), calm.Process(second)
    calm.close()
    r = make(up, down, T, "random")
    assert same(r.Process(first), y0)
    n = r.PredictOutputLen(second.shape[1])
    out = np.full((CH, n), np.nan)
    before = bits(out).copy()
    n_out = C.c_int64(-1)
    rc = lib().ad_resampler_process(r._h, ptr(second), second.shape[1], ptr(out), n - 1, C.byref(n_out))
    assert rc == _lib.AD_ERR_INVALID_ARGUMENT
    assert np.array_equal(bits(out), before)
    # device form: the same refusal, nothing written
    src, dst = LL.place(second, LL.L0, DEV), LL.empty(CH, n, LL.L0, DEV)
    sync()
    rc = lib().ad_resampler_process_device(r._h, C.c_void_p(src.ptr), src.stride, second.shape[1],
                                           C.c_void_p(dst.ptr), dst.stride, n - 1, C.byref(n_out), None)
    sync()
    assert rc == _lib.AD_ERR_INVALID_ARGUMENT
    LL.check_guards(dst, untouched=[(0, n)])
    assert r.PredictOutputLen(second.shape[1]) == n
    assert same(r.Process(second), y1)
    r.close()


def test_create_rejects_bad_prototypes(gpu):
    good = RR.random_taps(160, 16, 5)
    for bad in (np.nan, np.inf, -np.inf):
        t = good.copy()
        t[1234] = bad
        with pytest.raises(_lib.ErrInvalidArgument):
            R.NewRational(160, 147, taps=t)
    with pytest.raises(_lib.ErrInvalidArgument):
        R.NewRational(160, 147, taps=good[:-1])
    # the multiple is of the reduced up: 480 = 3 * 160 is taken for 320/294, 400 is not
    r = R.NewRational(320, 294, taps=np.ones(480))
    assert r.TapsPerPhase() == 3 and r.Ratio() == (160, 147)
    r.close()
    with pytest.raises(_lib.ErrInvalidArgument):
        R.NewRational(320, 294, taps=np.ones(400))
    with pytest.raises(_lib.ErrInvalidArgument):
        R.NewRational(160, 147, taps=np.zeros(0))
    with pytest.raises(_lib.ErrInvalidArgument):
        R.NewRational(160, 147, taps=good, channels=0)


def test_ratio_quality_and_prototype(gpu):
    r = R.NewRational(320, 294)
    assert r.Ratio() == (160, 147)
    assert r.Quality() == R.QualityBalanced and r.TapsPerPhase() == 32
    p = R.QualityProfile(R.QualityBalanced)
    assert same(r.Prototype(), R.design_polyphase_fir(160, 147, p.TapsPerPhase, p.CutoffScale, p.KaiserBeta))
    r.close()
    r = R.NewForRates(44100, 48000)
    assert r.Ratio() == (160, 147)
    r.close()
    r = R.NewRational(1, 2, quality=R.QualityBest, taps_per_phase=0, kaiser_beta=-1)
    assert r.Quality() == R.QualityBest and r.TapsPerPhase() == 64
    r.close()
    r = R.NewRational(3, 2, quality=R.QualityFast, taps_per_phase=24)
    assert r.TapsPerPhase() == 24 and r.Prototype().size == 72
    r.close()


def test_standard_ratios_length(gpu):
    """The reference's TestStandardRatios_Length (resample_test.go:51-79)."""
    for in_rate, out_rate in [(44100, 48000), (48000, 44100), (48000, 96000), (96000, 48000)]:
        r = R.NewForRates(in_rate, out_rate, quality=R.QualityBalanced)
        x = np.array([math.sin(2 * math.pi * 1000 * float(i) / in_rate) for i in range(4096)])
        y = r.Process(x)
        ref = RR.Ref(*r.Ratio(), r.Prototype()).process_vec(x)
        r.close()
        assert abs(len(y) - int(round(4096 * out_rate / in_rate))) <= 1
        assert same(y, ref)


def test_one_shot_helpers(gpu):
    x = signal(1500)
    p = R.QualityProfile(R.QualityFast)
    for fn, up, down in [(R.Upsample2x, 2, 1), (R.Downsample2x, 1, 2)]:
        h = R.design_polyphase_fir(up, down, p.TapsPerPhase, p.CutoffScale, p.KaiserBeta)
        w, _ = RR.resample(up, down, h, x)
        assert same(fn(x, quality=R.QualityFast), w)
        assert same(fn(x[0], quality=R.QualityFast), w[0])
    h = R.design_polyphase_fir(3, 2, 32, 0.92, 7.5)
    assert same(R.Resample(x[1], 6, 4), RR.resample(3, 2, h, x[1])[0][0])


# ------------------------------------------------------------ device layout
def test_process_device_layouts(gpu):
    """ad_resampler_process_device: 3 channels, 160/147, two consecutive calls
    of 1000 and 197 samples, input and output placed independently; the bits
    of the contiguous aligned call, clean guards, the input unchanged, and
    only n_out elements of each output row written."""
    up, down, T = 160, 147, 32
    x = signal(1500)
    calls = [np.ascontiguousarray(x[:, :1000]), np.ascontiguousarray(x[:, 1000:1197])]
    w, _ = want(up, down, T, "random", 1500)
    ref = RR.Ref(up, down, taps_for(up, down, T, "random"))
    n_outs = [len(ref.process_vec(c[0])) for c in calls]
    room = 40  # every output row is longer than n_out
    placements = [LL.LA, LL.L1, LL.L2, LL.L3]

    def lay(l, length):
        return l(length) if callable(l) else l

    base = None
    for lin in placements:
        for lout in placements:
            r = make(up, down, T, "random")
            got = []
            for blk, no in zip(calls, n_outs):
                n_in = blk.shape[1]
                src = LL.place(blk, lay(lin, n_in), DEV)
                dst = LL.empty(CH, no + room, lay(lout, no + room), DEV)
                sync()
                assert r.PredictOutputLen(n_in) == no
                assert r.process_device(src.ptr, src.stride, n_in, dst.ptr, dst.stride, no + room) == no
                sync()
                LL.check_unchanged(src, blk)
                LL.check_guards(dst, untouched=[(no, no + room)])
                got.append(LL.payload(dst)[:, :no])
            r.close()
            y = np.concatenate(got, axis=1)
            if base is None:
                base = y  # (LA, LA): the contiguous, 16-byte-aligned call
                assert same(base, w[:, :base.shape[1]])
            assert same(y, base), (lin, lout)


def test_process_device_refuses_overlap_and_short_strides(gpu):
    r = make(3, 2, 32, "random")
    n = 200
    no = r.PredictOutputLen(n)
    buf = LL.place(np.zeros((CH, n + no)), LL.L0, DEV)
    n_out = C.c_int64(-1)
    L = lib()
    sync()
    args = lambda i, istr, o, ostr: (r._h, C.c_void_p(i), istr, n, C.c_void_p(o), ostr, no, C.byref(n_out), None)
    # output rows inside the input rows' extent
    assert L.ad_resampler_process_device(*args(buf.ptr, buf.stride, buf.ptr + 8 * n, buf.stride)) \
        == _lib.AD_ERR_INVALID_ARGUMENT
    assert L.ad_resampler_process_device(*args(buf.ptr, n - 1, buf.ptr, no)) == _lib.AD_ERR_INVALID_ARGUMENT
    sync()
    LL.check_unchanged(buf)
    assert r.PredictOutputLen(n) == no  # nothing was taken in
    r.close()


# -------------------------------------------------------------- IR library
def test_library_provider_resamples_to_target_rate(gpu):
    """LibraryProvider(target_rate=44100): Large Church comes back resampled
    from 48000 by 147/160 at Balanced quality, all channels in one call."""
    plain = irlib.LibraryProvider()
    prov = irlib.LibraryProvider(target_rate=44100.0)
    idx = plain.IRNames().index("Large Church")
    s, rate, ok = plain.GetIR(idx)
    assert ok and rate == 48000.0
    y, new_rate, ok = prov.GetIR(idx)
    assert ok and new_rate == 44100.0
    p = R.QualityProfile(R.QualityBalanced)
    h = R.design_polyphase_fir(147, 160, p.TapsPerPhase, p.CutoffScale, p.KaiserBeta)
    w, _ = RR.resample(147, 160, h, s)
    assert y.shape == w.shape and y.shape[1] == -((-s.shape[1] * 147) // 160)
    assert same(y, w)
    assert prov.GetIR(idx)[0] is y  # resampled once
    assert prov.GetIR(-1) == (None, 0.0, False)
    # an IR already at the target rate, and the default provider, are returned as stored
    prov.target_rate = 48000.0
    assert prov.GetIR(idx)[0] is prov.irs[idx]["samples"] and prov.GetIR(idx)[1] == 48000.0
