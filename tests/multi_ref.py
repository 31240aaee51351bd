"""nmod_read_llr_multi (K26) restated in numpy from the text of include/nanomod_hip.h, on top of K13's restatement: plane m of llr and
llr_win, with its gates, is readllr_ref.restate for the pair (model, alt[m - 1]); the joint call, the posterior over the states and the
counts are restated here.  Also the seeded inputs the CPU and GPU tests share.  Nothing here calls the library.

Gates.  The planes are K13's (bit-equal on the device; the GPU test pins that), so their gates are K13's.  The posterior of state m moves
by at most sum_k |dL_k| relative when the window sums move by dL_k (d log post_m = dL_m - sum_k post_k dL_k and post <= 1), so its gate
is the sum of gate_L over the open planes, + GATE_P_EXTRA for the exp and the division: at n_alt = 1 exactly K13's p_mod gate."""
import functools

import numpy as np

import readllr_ref as F
import rescale_ref as R

MULTI_MAX = 4
AMBIGUOUS, NONE = 255, 254
TOO_LARGE = F.TOO_LARGE
MAX_DEEP = F.MAX_DEEP
WAVE_MAX = F.WAVE_MAX
GATE_P_EXTRA = F.GATE_P_EXTRA
LDS_PER_CU = 160 * 1024


def table_in_lds(n_alt, k):
    """read_llr_multi.hip's placement rule restated: the table (2 + 3 n_alt doubles per code) goes to LDS iff adding its bytes to the
    workgroup's stage (n_alt x 16 KiB + 256) leaves the workgroups a CU holds (at most 5) unchanged"""
    group = 8 * 4 * 512 * n_alt + 256
    res = lambda b: min(LDS_PER_CU // b, 5)
    return res(group + 4 ** k * (2 + 3 * n_alt) * 8) >= res(group)


def l2_side_k(n_alt):
    """the smallest k whose table is read through L2"""
    return next(k for k in range(1, 9) if not table_in_lds(n_alt, k))


def joint_call(L, thr):
    """the call of every event from its window sums L (n_alt x events, NaN: closed): uint8"""
    L = np.asarray(L, np.float64)
    n_alt, n = L.shape
    call = np.full(n, NONE, np.uint8)
    for j in range(n):
        open_ = [m for m in range(n_alt) if not np.isnan(L[m, j])]
        if not open_:
            continue
        b = open_[0]
        for m in open_[1:]:
            if L[m, j] > L[b, j]:
                b = m
        second = 0.0
        for m in open_:
            if m != b and L[m, j] > second:
                second = L[m, j]
        if L[b, j] - second >= thr:
            call[j] = b + 1
        elif all(L[m, j] <= -thr for m in open_):
            call[j] = 0
        else:
            call[j] = AMBIGUOUS
    return call


def joint_call_fast(L, thr):
    """joint_call without the Python loop over events (the GPU tests' batches); pinned to joint_call in tests/test_read_llr_multi.py"""
    L = np.asarray(L, np.float64)
    n_alt, n = L.shape
    open_ = ~np.isnan(L)
    some = open_.any(axis=0)
    low = np.where(open_, L, -np.inf)
    b = np.argmax(low, axis=0)                                   # the first of equal maxima: ties to the smaller m
    Lb = low[b, np.arange(n)]
    rest = low.copy()
    rest[b, np.arange(n)] = -np.inf
    second = np.maximum(rest.max(axis=0), 0.0)
    second = np.where(second > 0.0, second, 0.0)
    with np.errstate(invalid='ignore'):
        is_b = some & (Lb - second >= thr)
        is_can = some & ~is_b & np.where(open_, L <= -thr, True).all(axis=0)
    call = np.full(n, NONE, np.uint8)
    call[some] = AMBIGUOUS
    call[is_can] = 0
    call[is_b] = (b[is_b] + 1).astype(np.uint8)
    return call


def posterior(L, prior_logit):
    """post (n_alt + 1 x events) of the window sums L (n_alt x events) at the log prior odds of each state: the header's softmax"""
    L = np.asarray(L, np.float64)
    n_alt, n = L.shape
    open_ = ~np.isnan(L)
    some = open_.any(axis=0)
    prior = np.asarray(prior_logit, np.float64).reshape(n_alt, 1)
    u = L + prior
    mx = np.maximum(np.where(open_, u, -np.inf).max(axis=0), 0.0)
    mx = np.where(mx > 0.0, mx, 0.0)
    post = np.full((n_alt + 1, n), np.nan)
    with np.errstate(invalid='ignore', over='ignore'):
        e0 = np.exp(-mx)
        e = np.where(open_, np.exp(u - mx), 0.0)
        Z = e0.copy()
        for m in range(n_alt):                                       # ascending m
            Z = Z + e[m]
        post[0] = e0 / Z
        for m in range(n_alt):
            post[m + 1] = e[m] / Z
    post[:, ~some] = np.nan
    return post


def counts(call, off, n_alt):
    off = np.asarray(off, np.int64)
    nreads = len(off) - 1
    n_sites, n_can, n_mod = np.zeros(nreads, np.int32), np.zeros(nreads, np.int32), np.zeros((n_alt, nreads), np.int32)
    for i in range(nreads):
        c = call[off[i]:off[i + 1]]
        n_sites[i] = int((c != NONE).sum())
        n_can[i] = int((c == 0).sum())
        for m in range(n_alt):
            n_mod[m, i] = int((c == m + 1).sum())
    return n_sites, n_can, n_mod


def joint(L, off, thr, prior_logit, status=None):
    """everything the entry derives from its llr_win planes: dict(call, post, n_sites, n_can, n_mod); a TOO_LARGE read has NONE calls and
    NaN planes already (its L is NaN)"""
    L = np.asarray(L, np.float64)
    call = joint_call_fast(L, thr)
    n_sites, n_can, n_mod = counts(call, off, L.shape[0])
    return dict(call=call, post=posterior(L, prior_logit), n_sites=n_sites, n_can=n_can, n_mod=n_mod)


def restate(val, off, base, k, center, mean0, sd0, alts, window='kmer', thr=2.5, prior_logit=None):
    """the whole entry on host arrays.  alts: a sequence of (mean, sd).  dict(llr, llr_win, gate_llr, gate_L (n_alt x events), post,
    gate_post (n_alt + 1 x events, relative), call, n_sites, n_can, n_mod, status)"""
    n_alt = len(alts)
    prior_logit = np.zeros(n_alt) if prior_logit is None else np.asarray(prior_logit, np.float64)
    planes = [F.restate(val, off, base, k, center, mean0, sd0, m1, s1, window, thr, float(pl)) for (m1, s1), pl in zip(alts, prior_logit)]
    out = {f: np.stack([p[f] for p in planes]) for f in ('llr', 'llr_win', 'gate_llr', 'gate_L')}
    out.update(joint(out['llr_win'], off, thr, prior_logit))
    out['status'] = planes[0]['status']
    open_ = ~np.isnan(out['llr_win'])
    out['gate_post'] = np.broadcast_to(np.where(open_, out['gate_L'], 0.0).sum(axis=0) + GATE_P_EXTRA, out['post'].shape)
    out['p_mod'] = np.stack([p['p_mod'] for p in planes])
    return out


# ------------------------------------------------------------------------------------------------------------------ shared inputs

PARITY_THR = F.PARITY_THR
PARITY_PRIORS = (0.375, -1.25, 2.0, -0.5)
PARITY_DTYPES = F.PARITY_DTYPES


def windows_of(k, center):
    return ((0, 0), F.kmer_window(k, center), (64, 64))


def inner_of(window):
    return 512 - 8 * ((window[0] + 7) // 8) - 8 * ((window[1] + 7) // 8)


def parity_lengths(window):
    """1, 63, 64, 65, the tile's inner width +- 1, NMOD_CALLS_WAVE_MAX +- 1 (both kernel forms) and one read of 3 tiles per wave of the
    workgroup form (12 tiles, the last one partial)"""
    inner = inner_of(window)
    return [1, 63, 64, 65, inner - 1, inner, inner + 1, WAVE_MAX - 1, WAVE_MAX, WAVE_MAX + 1, 12 * inner - 5]


def make_alts(k, mean, sd, n_alt):
    """n_alt modified tables of a model: readllr_ref.make_alt_model under another seed each, and NaN entries that differ between the
    tables (k >= 2), so that the open sets differ along a read"""
    alts = []
    m = 4 ** k
    for a in range(n_alt):
        mean1, sd1 = F.make_alt_model(k, mean, sd, seed=9 + 31 * a, holes=a == 0)
        if k >= 2:
            mean1[(1 + 5 * a) % m] = np.nan
            sd1[(7 + 3 * a) % m] = np.nan
            mean1[(11 + a) % m] = np.inf
        alts.append((mean1, sd1))
    return alts


@functools.lru_cache(maxsize=None)
def parity_inputs(k, center, window, dtype, n_alt=MULTI_MAX):
    """the parity read set: dict(val, off, base, mean, sd, alts) — the lengths above, reads drawn from the unmodified table and from each
    modified table in turn, contaminated values and an 'N' in some reads.  The first n_alt of MULTI_MAX tables: the reads are the same
    for every n_alt"""
    window = tuple(window)
    rng = np.random.default_rng(2600 + 1000 * k + 100 * center + 7 * window[0] + window[1])
    mean, sd = R.make_model(k)
    alts = make_alts(k, mean, sd, MULTI_MAX)
    vals, bases = [], []
    for i, n in enumerate(parity_lengths(window)):
        src = (mean, sd) if i % 5 == 0 else alts[i % 5 - 1]
        src = (np.where(np.isfinite(src[0]), src[0], mean), np.where(np.isfinite(src[1]) & (src[1] > 0), src[1], sd))
        b, x = R.draw_read(rng, n, k, center, src[0], src[1], 0.0, 1.0, n_letters=2 if i % 3 == 0 else 0)
        vals.append(x); bases.append(b)
    lens = [len(v) for v in vals]
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    val = R.cast(np.concatenate(vals), dtype)
    for a in (val, off, mean, sd):
        a.setflags(write=False)
    return dict(val=val, off=off, base=np.concatenate(bases), mean=mean, sd=sd, alts=tuple(alts[:n_alt]))


def parity_cases():
    """(n_alt, k, center, window, dtype): k = 3 and the smallest k on the L2 side of the table switch (k = 2 as well where k = 3 is already
    there), the three windows, the three dtypes"""
    cases = []
    for n_alt in range(1, MULTI_MAX + 1):
        ks = sorted({3, l2_side_k(n_alt)} | ({2} if not table_in_lds(n_alt, 3) else set()))
        for k in ks:
            center = 1 if k >= 2 else 0
            for window in windows_of(k, center):
                for dtype in PARITY_DTYPES:
                    cases.append((n_alt, k, center, window, dtype))
    return cases


def chain_inputs(seed=78, n_reads=240, genome_len=700, shift_sd=3.0):
    """~240 reads of 300 .. 600 events drawn from a 3-mer model (center 0) over one short reference, both strands, and two modified tables:
    table 1 equals the unmodified one but at the k-mers that cover planted base A, whose levels lie shift_sd spreads higher; table 2 likewise
    at planted base B with levels shift_sd spreads LOWER.  Half of the reads carry state 1 at A, half of the reads carry state 2 at B
    (independently); at C both tables are shifted like that as well, but no read is: every read there is canonical.  (reads, model, [alt1, alt2], (A, B, C))"""
    k, center = 3, 0
    mean, sd = R.make_model(k, holes=False)
    rng = np.random.default_rng(seed)
    genome = rng.choice(np.frombuffer(b'ACGT', np.uint8), genome_len)
    sites = (genome_len // 2 - 12, genome_len // 2, genome_len // 2 + 12)
    lo, hi = F.kmer_window(k, center)
    means = [mean.copy(), mean.copy()]
    plan = []
    for r in range(n_reads):
        minus = r % 2 == 1
        n = int(rng.integers(300, 601))
        s0 = int(rng.integers(max(0, sites[2] - n + 20), min(genome_len - n, sites[0] - 20) + 1))
        pos = s0 + np.arange(n) if not minus else s0 + n - 1 - np.arange(n)
        b = genome[pos] if not minus else R._COMP[genome[pos]]
        codes = R.read_codes(b, k, center)
        covers = []
        for t, site in enumerate(sites[:2]):
            j = int(np.flatnonzero(pos == site)[0])
            cover = np.arange(j - lo, j + hi + 1)
            means[t][codes[cover]] = mean[codes[cover]] + (shift_sd if t == 0 else -shift_sd) * sd[codes[cover]]
            covers.append(cover)
        jc = int(np.flatnonzero(pos == sites[2])[0])                         # C: both tables differ from the unmodified one there, no read does
        cover = np.arange(jc - lo, jc + hi + 1)
        means[0][codes[cover]] = mean[codes[cover]] + shift_sd * sd[codes[cover]]
        means[1][codes[cover]] = mean[codes[cover]] - shift_sd * sd[codes[cover]]
        plan.append((minus, s0, b, codes, covers, rng.normal(size=n)))
    chrom, strand, start, vals, bases = [], [], [], [], []
    for r, (minus, s0, b, codes, covers, noise) in enumerate(plan):
        level = mean[codes].copy()
        if (r // 2) % 2 == 0:
            level[covers[0]] = means[0][codes[covers[0]]]
        if (r // 4) % 2 == 0:
            level[covers[1]] = means[1][codes[covers[1]]]
        chrom.append('chrT'); strand.append('-' if minus else '+'); start.append(s0); bases.append(b)
        vals.append(np.rint((level + sd[codes] * noise) * 1000.0) / 1000.0)
    off = np.zeros(n_reads + 1, np.int64)
    off[1:] = np.cumsum([len(v) for v in vals])
    reads = dict(chrom=np.array(chrom), strand=np.array(strand), start=np.array(start, np.int64), off=off,
                 norm_mean=R.cast(np.concatenate(vals), 'int16'), base=np.concatenate(bases).view('S1'))
    ones = np.ones(4 ** k, np.int64)
    model = dict(k=k, center=center, mean=mean, sd=sd, n_positions=ones)
    alts = [dict(k=k, center=center, mean=m1, sd=sd.copy(), n_positions=ones) for m1 in means]
    return reads, model, alts, sites
