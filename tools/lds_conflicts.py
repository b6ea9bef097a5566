"""Bank-conflict model of the LDS FFT passes (fft_device.hpp FftPlan, lds_slot).

Banking per /opt/skills/guides/MI355X_MICROARCH.md (§LDS): a ds_read_b128 is
served in four 16-lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31}, ... over
64 banks (16 slots of 16 B); a ds_write_b128 in eight groups of 8 contiguous
lanes over 32 banks (8 slots of 16 B).  Each extra distinct address on a busy
slot within a group costs one LDS cycle (SQ_LDS_BANK_CONFLICT counts them).

For every plan (M, V) at a workgroup of max(M/V, 256) threads, this prints the
extra cycles per workgroup of its Stockham stores and loads plus the
consecutive staging reads/writes, for the round-1 swizzle (AD_LDS_SWZ=0) and
the round-5 one (AD_LDS_SWZ=1), with unpadded (M) and padded (M + 1) rows.
Ahead of that table it prints the same figure for each exchange of the
long-block row kernel, which addresses its wave slices directly.

  python3 tools/lds_conflicts.py
"""
import collections

RD = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
      [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
RD += [[x + 32 for x in g] for g in RD]
WR = [list(range(8 * k, 8 * k + 8)) for k in range(8)]


def swz0(i):  # g(i >> 4) on the low 4 bits
    q = i >> 4
    return i ^ ((q ^ ((q & 4) << 1)) & 15)


def swz1(i):  # x(bits 3..6) from a packed 16-entry table
    t = (i >> 3) & 15
    return i ^ ((0xde0321fc12cfed30 >> (4 * t)) & 15)


def plan(M, V):
    LOG, LOGV = M.bit_length() - 1, V.bit_length() - 1
    NP = (LOG + LOGV - 1) // LOGV
    R0 = 1 << (LOG - LOGV * (NP - 1))
    return NP, R0, M // V


def patterns(M, V):
    """(kind, [(fft, index)] per thread) for each LDS instruction of one workgroup."""
    NP, R0, T = plan(M, V)
    LOGV = V.bit_length() - 1
    radix = lambda p: R0 if p == 0 else V
    ns = lambda p: 1 if p == 0 else R0 * (1 << (LOGV * (p - 1)))
    nt = max(T, 256)
    out = []
    for p in range(NP - 1):
        R, NS = radix(p), ns(p)
        for s in range(V):
            b, r = s // R, s % R
            out.append(('w', [(t // T, ((t % T + b * T) // NS) * NS * R + ((t % T + b * T) & (NS - 1)) + r * NS)
                              for t in range(nt)]))
        R1 = radix(p + 1)
        for s in range(V):
            b, r = s // R1, s % R1
            out.append(('r', [(t // T, t % T + b * T + r * (M // R1)) for t in range(nt)]))
    for s in range(V):
        out.append(('r', [(t // T, t % T + s * T) for t in range(nt)]))
        out.append(('w', [(t // T, t % T + s * T) for t in range(nt)]))
    return out


def extra_cycles(pats, rowoff, f):
    tot = 0
    for kind, ad in pats:
        groups, nslot = (RD, 16) if kind == 'r' else (WR, 8)
        for w in range(0, len(ad), 64):
            lanes = ad[w:w + 64]
            for g in groups:
                addrs = {lanes[l][0] * rowoff + f(lanes[l][1]) for l in g}
                per = collections.Counter(a % nslot for a in addrs)
                tot += max(per.values()) - 1
    return tot


def long_rows_patterns(xor=True):
    """k_long_rows (conv_long_kernels.hip): 512 threads, wave w owns the slice
    at 512 w.  name -> the eight writes and eight reads of each exchange of the
    forward (F) and inverse (I) transform; addresses are used as they are (no
    lds_slot).  xor=False drops the l ^ r of the two exchanges whose writers'
    eight-lane groups run over the slot digit, to show what it is for."""
    out = {}
    tids = range(512)
    wv = lambda t: 512 * (t >> 6)
    l0, l1, ln = (lambda t: t & 7), (lambda t: t & 56), (lambda t: t & 63)
    x = (lambda a, b: a ^ b) if xor else (lambda a, b: a)
    cross_w = lambda r: [(0, 512 * r + t) for t in tids]            # into / out of every slice
    plain_r = lambda r: [(0, wv(t) + 64 * r + ln(t)) for t in tids]
    mid_w = lambda r: [(0, wv(t) + 8 * l1(t) + 8 * r + l0(t)) for t in tids]
    xor_w = lambda r: [(0, wv(t) + 64 * l0(t) + x(l1(t) + r, l0(t))) for t in tids]
    xor_r = lambda r: [(0, wv(t) + 64 * r + x(ln(t), r)) for t in tids]
    for name, w, r in [("F pass 0 -> 1 (workgroup)", cross_w, plain_r), ("F pass 1 -> 2", mid_w, plain_r),
                       ("F pass 2 -> 3", xor_w, xor_r), ("I pass 0 -> 1", xor_w, xor_r),
                       ("I pass 1 -> 2", mid_w, plain_r), ("I pass 2 -> 3 (workgroup)", plain_r, cross_w)]:
        out[name] = [('w', w(s)) for s in range(8)] + [('r', r(s)) for s in range(8)]
    return out


def check_long_rows_exchange():
    """Each exchange's writes cover the image once and its reads the same cells."""
    for name, p in long_rows_patterns().items():
        writes = [a for s in range(8) for (_, a) in p[s][1]]
        reads = [a for s in range(8) for (_, a) in p[8 + s][1]]
        assert sorted(writes) == sorted(reads) == list(range(4096)), name


if __name__ == "__main__":
    print("k_long_rows exchanges (extra LDS cycles per workgroup; without the lane ^ slot swizzle in brackets)")
    check_long_rows_exchange()
    ident = lambda i: i
    plain = long_rows_patterns(False)
    for name, p in long_rows_patterns().items():
        print(f"  {name:28s} {extra_cycles(p, 0, ident):5d}  [{extra_cycles(plain[name], 0, ident)}]")
    print()
    print(f"{'plan':>12}  {'rows':>5}  {'swz0':>6}  {'swz1':>6}   (extra LDS cycles per workgroup)")
    for M, V in [(8192, 8), (4096, 8), (2048, 8), (1024, 8), (512, 8), (256, 8), (256, 4), (1024, 4),
                 (4096, 16), (2048, 16), (1024, 16), (512, 16), (256, 16)]:
        pats = patterns(M, V)
        for ro in (M, M + 1):
            print(f"M={M:5d} V={V:2d}  {ro - M:>+5d}  {extra_cycles(pats, ro, swz0):6d}  {extra_cycles(pats, ro, swz1):6d}")
