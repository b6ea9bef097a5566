"""CPU proof of tests/conv_exact.py: the exact references agree with each
other and with the C oracle's long-double sum, every integer case stays exact,
and the case lists reach every plan of the engine.  The same run measures
gamma_ref: the worst error / err_scale of conv_exact.upols_numpy (the engine's
algorithm on numpy's fp64 FFT) per hop over the cases the GPU sweep runs,
which test_conv_plans_gpu.py's bound is 8 times, and the C oracle's figure
next to it.  Two perturbations of the numpy restatement (one spectrum bin of
one partition times 1 + 1e-11; one partition's spectrum rounded through
complex64) show that errors the older 1e-7 RMS / 1e-9 bars accept break the new
bound at every hop.  No GPU, under a minute.
"""
import numpy as np
import pytest

import conv_exact as E
import oracle_lib as O

# Worst error / err_scale per hop, measured by test_gamma_ref_* below when this
# file was written (numpy 2.x pocketfft; the C oracle = liboracle's FFT
# convolutions).  "part": the partitioned handles (a sum over stages).  A run
# that measures more than the figure here fails.
GAMMA_REF = {64: 1.12, 128: 1.25, 256: 1.44, 512: 1.31, 1024: 1.27, 2048: 1.11, 4096: 1.21, 8192: 1.31, "part": 1.18}
ORACLE_REF = {64: 1.14, 128: 1.36, 256: 1.22, 512: 1.25, 1024: 1.36, 2048: 1.46, 4096: 1.42, 8192: 1.46, "part": 1.26}
# a correct fp64 FFT convolution stays within a few err_scale; a wrong index or
# convention gives 10^10 and more
SANE = 4.0
OLD_RMS, OLD_MAX = 1e-7, 1e-9  # the suite's older bars (FFT_RMS_TOL, max |got - want|)


def _ratio(got, exact, scale):
    assert got.shape == exact.shape
    err = float(np.max(np.abs(got - exact))) if exact.size else 0.0
    return err / scale if scale > 0 else (0.0 if err == 0 else float("inf"))


class _Worst(dict):
    def add(self, who, key, name, got, exact, scale):
        r = _ratio(got, exact, scale)
        assert r <= SANE, f"{who} hop={key} {name}: {r:.3g} err_scale"
        self[(who, key)] = max(self.get((who, key), 0.0), r)

    def report(self, keys):
        for k in keys:
            n, o = self.get(("numpy", k), 0.0), self.get(("oracle", k), 0.0)
            print(f"GAMMA_REF hop={k} numpy={n:.3f} oracle={o:.3f} recorded={GAMMA_REF[k]} / {ORACLE_REF[k]}")
        for k in keys:
            n, o = self.get(("numpy", k), 0.0), self.get(("oracle", k), 0.0)
            assert n <= GAMMA_REF[k], f"hop {k}: numpy measures {n:.3f}, recorded gamma_ref {GAMMA_REF[k]}"
            assert o <= ORACLE_REF[k], f"hop {k}: the C oracle measures {o:.3f}, recorded {ORACLE_REF[k]}"


def _ols(case):
    return O.OverlapSave(case.h, 0).process(case.x)[: case.exact.size]


# ------------------------------------------------------------ the references
def test_references_agree():
    """Sparse sum = np.convolve on int64 = direct_ld (equal, or 2^-60 relative)
    at small sizes, in both roles; the shifts against direct_ld."""
    for L, K, n in [(64, 133, 401), (128, 128, 300), (64, 61, 64), (256, 517, 1000)]:
        hpos, hval = E.sparse_int(K, L, 11 + K, E.DENSE_INT_RANGE)
        xi = E.dense_int(n, 12 + K, E.DENSE_INT_RANGE)
        h = E.densify(hpos, hval, K)
        sp, partial = E.sparse_convolve(hpos, hval, xi)
        dense = E.int_convolve(xi, h.astype(np.int64))
        assert np.array_equal(sp, dense) and partial < 2**53
        ld = O.direct_ld(xi.astype(np.float64), h)
        assert np.max(np.abs(ld - dense)) <= 2.0**-60 * np.max(np.abs(dense))
        # the mirror: sparse input, dense kernel
        c = E.case_sparse_input(n, L, E.dense_int(K, 13 + K, E.DENSE_INT_RANGE), 14 + K)
        assert np.array_equal(c.exact, E.int_convolve(c.x.astype(np.int64), c.h.astype(np.int64)))
        # cut to out_len
        cut, _ = E.sparse_convolve(hpos, hval, xi, n)
        assert np.array_equal(cut, dense[:n])
        for c in (E.case_kernel_impulse(n, K, K - 1, 0.125, 15), E.case_kernel_impulse(n, K, 0, 4.0, 16),
                  E.case_input_impulse(n, E.noise(K, 17), min(L + 3, n - 2), 32.0),
                  E.case_input_impulse(n, E.noise(K, 18), n - 1, 0.5)):
            ld = O.direct_ld(c.x, c.h)
            assert np.max(np.abs(ld - c.exact)) <= 2.0**-60 * c.peak


def test_sparse_positions_hit_every_boundary():
    for L in E.HOPS:
        for _, P, K, n in E.multi_variants(L):
            pos = set(E.boundary_positions(K, L, 1).tolist())
            assert len(pos) <= E.MAX_TAPS
            want = {0, K - 1} | {b * L + d for b in range(1, P) for d in (-1, 0, 1)}
            assert {p for p in want if 0 <= p < K} <= pos, (L, P)
    for L, P in E.BIG_P:  # 3 (P - 1) > 64: the first, last and group-of-16 boundaries, the rest drawn
        K = (P - 1) * L + 5
        pos = set(E.boundary_positions(K, L, 1).tolist())
        assert len(pos) <= E.MAX_TAPS and {0, K - 1} <= pos
        for b in (1, 16, 17, P - 1):
            assert {b * L - 1, b * L, b * L + 1} <= pos | {K}


def _all_integer_cases():
    for L in E.HOPS:
        for _, P, K, n in E.multi_variants(L):
            yield from E.multi_engines(L, P, K, n)[1][2]
        K = 3 * L + 5
        yield E.stream_cases(L, K, L)[2]
    for L, P in E.BIG_P:
        yield E.big_p_case(L, P)[2]
    for L, P in sorted({(L, P) for L, P, _ in E.MIX_CASES}):
        yield from E.mix_engine(L, P)[3]
    for lo in E.PART_LO:
        o = O.Partitioned(np.ones(E.part_kernel_len(lo)), lo, E.PART_HI)
        yield E.part_case(lo, [o.stage_info(i) for i in range(o.stage_count())], 40 + lo)[2]
    yield E.carried_case()[2]
    for B in E.MULTI_STREAM_B:
        yield from E.multi_stream_engine(B)[4][:2]
    for K in E.BATCH_K:
        yield E.batch_cases(K)[1][0]
    yield E.stream_cases(4096, 3 * 4096 + 5, 4096, E.F32_INT_RANGE)[2]


def test_integer_cases_stay_exact():
    """Every integer case's largest partial sum is below 2^53 (below 2^37 in
    fact: 64 taps of 2^15 against 2^15); the float32 handles' outputs are
    integers below 2^24."""
    count = 0
    for c in _all_integer_cases():
        assert c.partial > 0 and c.partial < 2**53 and c.partial < 2**37, (c.family, c.partial)
        assert np.array_equal(c.exact, np.round(c.exact))
        count += 1
    assert count > 150
    c = E.stream_cases(4096, 3 * 4096 + 5, 4096, E.F32_INT_RANGE)[2]
    assert c.peak < 2**24 and np.array_equal(c.exact.astype(np.float32).astype(np.float64), c.exact)


def test_err_scale_reduces_to_the_spectral_one():
    """One partition, one block: spectral_exact.err_scale at N = M = 2L."""
    import spectral_exact as X

    L = 256
    x, h = E.noise(L // 2, 1), E.noise(L // 2, 2)
    got = E.err_scale(x, h, L, 3.0)
    assert got == pytest.approx(X.err_scale(2 * L, X.norm2(x), X.norm2(h), 3.0), rel=1e-14)


# ------------------------------------------------------------------ gamma_ref
def test_gamma_ref_uniform_engine():
    """Entries a, b, c, e, f of the GPU sweep through upols_numpy (all of
    them) and the C oracle's OverlapSave / Streaming (P <= 17)."""
    w = _Worst()
    for L in E.HOPS:
        for name, P, K, n in E.multi_variants(L):
            for tag, _, chans in E.multi_engines(L, P, K, n, O.direct_ld):
                for i, c in enumerate(chans):
                    w.add("numpy", L, f"{name} {tag} ch{i} {c.family}", E.upols_numpy(c.x, c.h, L), c.exact, c.scale(L))
                    if i == 1 or c.family == "dense-float":
                        w.add("oracle", L, f"{name} {tag} ch{i} {c.family}", _ols(c), c.exact, c.scale(L))
        K = 3 * L + 5
        for c in E.stream_cases(L, K, L):
            n = c.exact.size
            w.add("numpy", L, f"stream {c.family}", E.upols_numpy(c.x, c.h, L, n), c.exact, c.scale(L))
            s = O.Streaming(c.h, L, ola=c.family == "sparse-kernel")
            got = np.concatenate([s.process_block(c.x[i: i + L]) for i in range(0, n, L)])
            w.add("oracle", L, f"stream {c.family}", got, c.exact, c.scale(L))
    K, n, c = E.big_p_case(2048, 256)
    w.add("numpy", 2048, "P=256", E.upols_numpy(c.x, c.h, 2048), c.exact, c.scale(2048))
    K, n, c = E.big_p_case(2048, 257)
    w.add("numpy", 2048, "P=257", E.upols_numpy(c.x, c.h, 2048), c.exact, c.scale(2048))
    for L, P in sorted({(L, P) for L, P, _ in E.MIX_CASES}):
        K, n, _, chans = E.mix_engine(L, P)
        got = [E.upols_numpy(c.x, c.h, L) for c in chans]
        for parity in (0, 1):
            for side, (exact, scale) in enumerate(E.mix_sides(chans, L, parity)):
                mine = [g for i, g in enumerate(got) if (parity + i) % 2 == side]
                w.add("numpy", L, f"mix P={P} side={side}", sum(mine, np.zeros(exact.size)), exact, scale)
    for B in E.MULTI_STREAM_B:
        L, K, n, _, chans = E.multi_stream_engine(B)
        for c in chans:
            w.add("numpy", L, f"multi-stream B={B} {c.family}", E.upols_numpy(c.x, c.h, L, n), c.exact, c.scale(L))
    L, _, c = E.carried_case()
    w.add("numpy", L, "carried", E.upols_numpy(c.x, c.h, L, c.exact.size), c.exact, c.scale(L))
    for K in E.BATCH_K:
        L, cases = E.batch_cases(K)
        for c in cases:
            w.add("numpy", L, f"batch K={K} {c.family}", E.upols_numpy(c.x, c.h, L), c.exact, c.scale(L))
            w.add("oracle", L, f"batch K={K} {c.family}", _ols(c), c.exact, c.scale(L))
    c = E.stream_cases(4096, 3 * 4096 + 5, 4096, E.F32_INT_RANGE)[2]
    w.add("numpy", 4096, "float32 stream", E.upols_numpy(c.x, c.h, 4096, c.exact.size), c.exact, c.scale(4096))
    w.report(E.HOPS)


def _staged_numpy(case, stages, lat):
    n = case.x.size
    y = np.zeros(n + lat)
    for p, T, cap in stages:
        taps = case.h[T: T + cap]
        if taps.size:
            part = E.upols_numpy(case.x, taps, p, n)
            y[lat + T:] += part[: n - T] if T < n else 0.0
    return y[:n]


def test_gamma_ref_partitioned():
    """Entry d (and g's partitioned handle): the staged algorithm on numpy's
    FFT over the stages StageInfo reports, and the C oracle's Partitioned."""
    w = _Worst()
    for lo, rng_ in [(lo, E.INT_RANGE) for lo in E.PART_LO] + [(7, E.F32_INT_RANGE)]:
        K = E.part_kernel_len(lo)
        o = O.Partitioned(np.ones(K), lo, E.PART_HI)
        info = [o.stage_info(i) for i in range(o.stage_count())]
        assert info[-1][0] == 1 << E.PART_HI  # the order-13 stage exists in the layout StageInfo reports ...
        stages = E.reference_stages(info)
        assert E.device_stages(K, lo, E.PART_HI)[-1][1] == K - 5  # ... and K is just past its start on the device
        if K > 5 + (1 << lo):  # ... and at no shorter kernel (one latency block fewer) in either layout
            o2 = O.Partitioned(np.ones(K - (1 << lo)), lo, E.PART_HI)
            assert o2.stage_info(o2.stage_count() - 1)[0] < 1 << E.PART_HI
            assert E.device_stages(K - 5, lo, E.PART_HI)[-1][0] < 1 << E.PART_HI
        K2, sizes, case, scale = E.part_case(lo, info, 40 + lo, rng_)
        assert K2 == K
        w.add("numpy", "part", f"lo={lo}", _staged_numpy(case, stages, 1 << lo), case.exact, scale)
        o = O.Partitioned(case.h, lo, E.PART_HI)
        pos, got = 0, []
        for m in sizes:
            got.append(o.process_block(case.x[pos: pos + m]))
            pos += m
        w.add("oracle", "part", f"lo={lo}", np.concatenate(got), case.exact, scale)
    w.report(["part"])


# ------------------------------------------------------------ the bound bites
def _perturbed(case, L, kind):
    H = E.partition_spectra(case.h, L)
    if kind == "bin":  # the strongest partition
        H[int(np.argmax(np.sum(np.abs(H) ** 2, axis=1))), L // 3] *= 1.0 + 1e-11
    else:  # the last partition
        H[-1] = H[-1].astype(np.complex64).astype(np.complex128)
    return E.upols_numpy(case.x, case.h, L, H=H)


@pytest.mark.parametrize("kind", ["bin", "complex64"])
def test_bound_has_teeth(kind):
    """One bin of one partition's spectrum times 1 + 1e-11, and one partition's
    spectrum rounded through complex64, on the numpy restatement: at every
    hop at least one case passes the older bars (1e-7 RMS, 1e-9 max) and
    exceeds 8 gamma_ref err_scale.  Unperturbed, every case is within
    gamma_ref err_scale."""
    for L in E.HOPS:
        hits, seen = [], []
        for c in E.teeth_cases(L):
            clean = E.upols_numpy(c.x, c.h, L)
            bound = 8.0 * GAMMA_REF[L] * c.scale(L)
            assert np.max(np.abs(clean - c.exact)) <= GAMMA_REF[L] * c.scale(L)
            d = _perturbed(c, L, kind) - c.exact
            old_ok = float(np.sqrt(np.mean(d * d))) < OLD_RMS and float(np.max(np.abs(d))) < OLD_MAX
            over = float(np.max(np.abs(d))) / bound
            seen.append(f"{c.family}: old bars {'pass' if old_ok else 'FAIL'}, error/bound {over:.3g}")
            hits.append(old_ok and over > 1.0)
        print(f"TEETH kind={kind} hop={L} " + "; ".join(seen))
        assert any(hits), (kind, L, seen)


# ----------------------------------------------------------- plan coverage
def test_sweep_reaches_every_plan():
    """The case lists (shared with the GPU sweep) reach every hop, all five PC
    instances with and without a tail, both MAC layouts at the split sizes,
    the ring wrap, the gated chain, the carried block and every batch hop."""
    for L in E.HOPS:
        vs = E.multi_variants(L)
        assert {P for _, P, _, _ in vs} == set(E.MULTI_P)
        assert {E.pick_pc(P) for _, P, _, _ in vs} == {1, 2, 4, 8, 16}
        assert any(P > 16 for _, P, _, _ in vs)
        for _, P, K, n in vs:
            assert E.n_partitions(K, L) == P
        assert any(K == L for _, _, K, _ in vs) and any(K == L + 1 for _, _, K, _ in vs)
        name, P, K, n = vs[-1]
        assert -(-(n + K - 1) // L) > E.ring_rows(P, E.MULTI_CHUNK)  # the ring wraps inside the call
        assert E.stream_hop(L, 3 * L + 5) == (L, False)
        assert E.stream_gated(L, 3 * L + 5) == (L >= 2048)
    assert {(L, E.mid_in_k3(L, P)) for L, P in E.BIG_P} == {(2048, True), (2048, False), (4096, False), (8192, False)}
    assert E.stream_hop(*E.STREAM_CARRIED) == (2048, True) and not E.stream_gated(*E.STREAM_CARRIED)
    assert [E.multi_stream_engine(B)[0] for B in E.MULTI_STREAM_B] == [256, 1024]
    assert E.stream_hop(1000, 3 * 1024 + 5, multi=True) == (1024, True)
    assert [E.batch_hop(K) for K in E.BATCH_K] == [256, 1024, 8192] and E.batch_hop(1) == 256
    assert {L for L, _, _ in E.MIX_CASES} == {1024, 2048, 4096, 8192}
    for lo in E.PART_LO:
        st = E.device_stages(E.part_kernel_len(lo), lo, E.PART_HI)
        assert st[-1][0] == 8192 and st[-1][2] == 5
        if lo <= 10:
            assert any(E.stage_fused(p, t) for p, _, t in st) and any(not E.stage_fused(p, t) for p, _, t in st)
