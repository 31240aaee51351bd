"""K-mer level models from a control run (K10; include/nanomod_hip.h: nmod_kmer_model).

A *k-mer model* is a table of 4^k entries: the expected level and spread of an event whose position sits at offset `center` of that
k-mer, in read direction.  It is what one-sample detection's 'model' kind of profile (onesample.py) is made from, and it is what
lets a control of one genome serve a sample of another, or a control that covers only part of the genome serve the rest:

    model = build_kmer_model(container.load_group('control.npz'), k=5, center=2, min_coverage=5)
    save_kmer_model('control_kmer_model.npz', model)
    prof = model_profile(model, container.load_group('sample.npz'))       # a kind-'model' profile of the sample's positions
    onesample.mtest1({... 'nmod_profile': prof ...})

A second table, the MODIFIED one that readllr's --altModel takes, is either built the same way from a fully modified control or learnt
from a mixed (native, partly modified) sample against the control's table (K17, nmod_kmer_mix):

    alt, table = learn_alt_model(container.load_group('native.npz'), model)
    save_kmer_model('native_alt_kmer_model.npz', alt)

The pooling runs in the HIP library; there is no CPU fallback.  Events are int16-exact (3-decimal), and that is the streaming form
of the device entry; float32 / float64 rows are reduced too, by a form that is not tuned.
"""
from __future__ import annotations

import numpy as np

from . import _lib as L
from . import container, detect, engine, onesample

KMER_MODEL_VERSION = 1
KMER_MODEL_FIELDS = ('version', 'k', 'center', 'clip_sigma', 'n_positions', 'n_samples', 'n_clipped', 'mean', 'sd')
MAX_K = 8


def _check_k(k, center):
    k, center = int(k), int(center)
    if not 1 <= k <= MAX_K:
        raise ValueError('k must be in 1 .. %d' % MAX_K)
    if not 0 <= center < k:
        raise ValueError('center must be in 0 .. k - 1')
    return k, center


def kmer_codes(chrom, strand, pos, base, k, center):
    """int32 code of the k-mer every row sits in, for rows in the reference's order (sorted (chrom, strand), ascending position).
    The k-mer of a position is the bases at read-direction offsets -center .. k - 1 - center, all inside its run of consecutive
    positions (detect.run_ids); the read-direction successor of a position is pos + 1 on '+' and pos - 1 on '-' (a '-' read's first
    event lies at its highest position, and `base` is the read's own base).  A = 0, C = 1, G = 2, T = 3, the first base most
    significant; any other letter, or a window that leaves the run, gives -1."""
    k, center = _check_k(k, center)
    pos = np.asarray(pos, dtype=np.int64)
    n = len(pos)
    if n == 0:
        return np.zeros(0, np.int32)
    first = engine._first_chars(np.asarray(base))
    val = np.full(256, -1, np.int64)
    val[[ord(c) for c in 'ACGT']] = np.arange(4)
    v = val[np.frombuffer(first, dtype=np.uint8)]
    rid = detect.run_ids(chrom, strand, pos).astype(np.int64)
    step = np.where(np.asarray(strand).astype(str) == '-', -1, 1).astype(np.int64)
    idx = np.arange(n, dtype=np.int64)
    code = np.zeros(n, np.int64)
    ok = np.ones(n, bool)
    for d in range(-center, k - center):
        j = idx + d * step
        inside = (j >= 0) & (j < n)
        jc = np.where(inside, j, 0)
        good = inside & (rid[jc] == rid) & (v[jc] >= 0)
        ok &= good
        code = code * 4 + np.where(good, v[jc], 0)
    return np.where(ok, code, -1).astype(np.int32)


def kmer_string(code, k):
    """the k-mer a code stands for"""
    return ''.join('ACGT'[(int(code) >> (2 * (k - 1 - i))) & 3] for i in range(k))


def group_codes(group, k, center):
    """kmer_codes for the rows of a per-position group in the group's OWN row order"""
    from . import cli
    n = len(group['pos'])
    names, (cid,) = cli._chrom_codes(group['chrom'])
    g = dict(strand=np.asarray(group['strand']).astype(str), pos=np.asarray(group['pos'], dtype=np.int64))
    rows, _ = onesample._sorted_rows(g, np.arange(n, dtype=np.int64), cid)
    codes = np.full(n, -1, np.int32)
    codes[rows] = kmer_codes(cid[rows], g['strand'][rows], g['pos'][rows], np.asarray(group['base'])[rows], k, center)
    return codes


def _encode(sig):
    """int16 milli-units where that is exact (the streaming form of the device entry), else onesample's choice"""
    sig = np.asarray(sig)
    if sig.dtype != np.int16 and sig.dtype.kind == 'f' and sig.size <= detect.DEVICE_ENCODE_ABOVE:
        m = container.milli_or_same(sig)
        if m.dtype == np.int16:
            return np.ascontiguousarray(m)
    return onesample._encode(sig)


_DROP_REASONS = ((L.STATUS_EMPTY, 'empty'), (L.STATUS_TOO_LARGE, 'beyond %d reads' % L.MAX_DEEP), (L.STATUS_NONFINITE, 'non-finite samples'))


def build_kmer_model(group, k=5, center=2, min_coverage=5, clip_sigma=0.0, clip_rounds=2, device=0, log=print):
    """The k-mer model of one read group (a per-position container: chrom, strand, pos, base, off, sig).  The contexts come from
    all rows of the group; the samples only from rows with at least min_coverage reads.  clip_sigma > 0: after the plain pass,
    clip_rounds more passes keep, per k-mer, the samples within mean +- clip_sigma * sd of the previous pass (a k-mer without an
    estimate keeps everything).  Returns a dict of KMER_MODEL_FIELDS; the arrays have 4^k entries (mean / sd NaN for a k-mer that
    was not seen)."""
    k, center = _check_k(k, center)
    clip_sigma, clip_rounds = float(clip_sigma), int(clip_rounds)
    if not clip_sigma >= 0.0 or clip_rounds < 0:
        raise ValueError('clip_sigma and clip_rounds must not be negative')
    ncodes = 4 ** k
    off = np.ascontiguousarray(group['off'], dtype=np.int64)
    codes = group_codes(group, k, center)
    no_context = int((codes < 0).sum())
    thin = (np.diff(off) < min_coverage) & (codes >= 0)
    codes[thin] = -1
    sig = _encode(group['sig']) if len(codes) else np.zeros(0, np.int16)
    res = engine.kmer_model_host(sig, off, codes, ncodes, device=device)
    for _ in range(clip_rounds if clip_sigma > 0.0 else 0):
        have = np.isfinite(res['mean']) & np.isfinite(res['sd'])
        lo = np.where(have, res['mean'] - clip_sigma * res['sd'], -np.inf)
        hi = np.where(have, res['mean'] + clip_sigma * res['sd'], np.inf)
        res = engine.kmer_model_host(sig, off, codes, ncodes, lo, hi, device=device)
    st = res['pos_status']
    dropped = ', '.join('%d %s' % (int(((st & bit) != 0).sum()), what) for bit, what in _DROP_REASONS if ((st & bit) != 0).any())
    log('kmer model: k = %d, %d of %d k-mers seen, %d position(s) pooled; dropped: %d without a full k-mer, %d below MinCoverage%s'
        % (k, int((res['n_positions'] > 0).sum()), ncodes, int(res['n_positions'].sum()), no_context, int(thin.sum()),
           (', ' + dropped) if dropped else ''))
    return dict(version=np.int32(KMER_MODEL_VERSION), k=np.int32(k), center=np.int32(center), clip_sigma=np.float64(clip_sigma),
                n_positions=res['n_positions'], n_samples=res['n_samples'], n_clipped=res['n_clipped'], mean=res['mean'], sd=res['sd'])


def save_kmer_model(path, model):
    """A k-mer model as an uncompressed .npz (KMER_MODEL_FIELDS); numpy appends '.npz' to a path without it."""
    np.savez(path, **{f: np.asarray(model[f]) for f in KMER_MODEL_FIELDS})


def load_kmer_model(path):
    with np.load(path) as z:
        if any(f not in z.files for f in KMER_MODEL_FIELDS) or int(z['version']) != KMER_MODEL_VERSION:
            raise ValueError('%s: not a version-%d k-mer model' % (path, KMER_MODEL_VERSION))
        model = {f: z[f] for f in KMER_MODEL_FIELDS}
    k = int(model['k'])
    if not 1 <= k <= MAX_K or not 0 <= int(model['center']) < k or any(len(model[f]) != 4 ** k for f in KMER_MODEL_FIELDS[4:]):
        raise ValueError('%s: inconsistent k-mer model' % path)
    return model


def write_kmer_table(path, model):
    """<FileID>_kmer_model.txt: per k-mer 'kmer n_positions n_samples mean sd' as '%s %d %d %.6f %.6f' (Python's spelling of nan)"""
    k = int(model['k'])
    cols = [np.asarray(model[f]).tolist() for f in ('n_positions', 'n_samples', 'mean', 'sd')]
    with open(path, 'w') as f:
        f.writelines('%s %d %d %.6f %.6f\n' % ((kmer_string(c, k),) + row) for c, row in enumerate(zip(*cols)))


KMER_MIX_COLUMNS = ('kmer', 'n_positions', 'n_used', 'n_outside', 'mean0', 'sd0', 'pi', 'mu_mod', 'sd_mod', 'llr', 'iters', 'status', 'kept')


def _listed_rows(group, sites):
    """which rows of a per-position group are among `sites` ((chrom, strand, pos) arrays, pos 0-based)"""
    chrom, strand, pos = (np.asarray(x) for x in sites)
    if not (len(chrom) == len(strand) == len(pos)):
        raise ValueError('sites: chrom, strand and pos need one entry per site')
    n = len(group['pos'])
    _, inv = np.unique(np.concatenate([np.asarray(group['chrom']).astype(str), chrom.astype(str)]), return_inverse=True)
    minus = np.concatenate([np.asarray(group['strand']).astype(str), strand.astype(str)]) == '-'
    key = ((inv.astype(np.int64) * 2 + minus) << 40) | np.concatenate([np.asarray(group['pos'], dtype=np.int64), pos.astype(np.int64)])
    return np.isin(key[:n], key[n:])


def select_alt_codes(res, mean0, sd0, min_samples=1000, min_pi=0.05, min_shift=1.0):
    """The codes of a kmer_mix result whose modified component goes into the table: the status has none of L.KMIX_DEGENERATE /
    TOO_FEW / NO_MODEL, n_used >= min_samples, pi >= min_pi and |mu_mod - mean0| >= min_shift * sd0.  By effect size, not by llr: at
    the pooled sample sizes of a k-mer any second component has a large llr (include/nanomod_hip.h).  L.KMIX_NOT_CONVERGED does not
    exclude a code."""
    with np.errstate(invalid='ignore'):
        return ((np.asarray(res['status']) & L.KMIX_NO_ESTIMATE) == 0) & (np.asarray(res['n_used']) >= min_samples) & \
               (np.asarray(res['pi']) >= min_pi) & (np.abs(np.asarray(res['mu_mod']) - mean0) >= min_shift * sd0)


def alt_model_from(model, res, kept):
    """the version-1 k-mer model of the kept codes' modified components: mean / sd NaN elsewhere (a NaN entry is an unusable code to
    every --altModel), n_samples = n_used, n_clipped = n_outside, clip_sigma 0"""
    kept = np.asarray(kept, dtype=bool)
    return dict(version=np.int32(KMER_MODEL_VERSION), k=np.int32(model['k']), center=np.int32(model['center']), clip_sigma=np.float64(0.0),
                n_positions=np.asarray(res['n_positions'], dtype=np.int64), n_samples=np.asarray(res['n_used'], dtype=np.int64),
                n_clipped=np.asarray(res['n_outside'], dtype=np.int64),
                mean=np.where(kept, res['mu_mod'], np.nan).astype(np.float64), sd=np.where(kept, res['sd_mod'], np.nan).astype(np.float64))


def learn_alt_model(group, model, sites=None, min_coverage=5, mix_model='free', max_iter=200, tol=1e-6, min_samples=1000, min_pi=0.05,
                    min_shift=1.0, device=0, log=print):
    """The MODIFIED k-mer model learnt from a mixed sample (K17, nmod_kmer_mix): `group` is the per-position container of a native,
    partly modified sample, `model` the k-mer model of an unmodified control (build_kmer_model).  Per k-mer the unmodified component is
    fixed at the control's entry, the events of the k-mer's positions are pooled, and y ~ (1 - pi) N(mean0, sd0^2) + pi N(m, v) is
    fitted on the device (mix_model 'free': v free, 'equal': v = sd0^2).  The codes come from group_codes; positions below
    min_coverage reads take no part, and with `sites` ((chrom, strand, pos) arrays, pos 0-based: what readllr.read_sites_file returns
    for the first three columns of a _sign_test.txt, _sign_test_fdr.txt or _site_stoich.txt) neither do the positions not listed — so
    only positions `detect` flagged may be pooled.
    A k-mer is KEPT by select_alt_codes(min_samples, min_pi, min_shift).  The three thresholds are defaults of judgement, not
    measurements: 1 000 events, a twentieth of the events, one control sd.  pi is the share over all pooled events of the k-mer, not
    per site (that is K14's job, with the learnt table).
    Returns (alt, table): alt a dict of KMER_MODEL_FIELDS (alt_model_from) that save_kmer_model and every --altModel take as it is;
    table every per-code output of the fit, mean0, sd0 and `kept`."""
    k, center = _check_k(model['k'], model['center'])
    ncodes = 4 ** k
    mean0, sd0 = np.asarray(model['mean'], dtype=np.float64), np.asarray(model['sd'], dtype=np.float64)
    if mean0.shape != (ncodes,) or sd0.shape != (ncodes,):
        raise ValueError('model mean / sd must be float64[4^k]')
    off = np.ascontiguousarray(group['off'], dtype=np.int64)
    codes = group_codes(group, k, center)
    no_context = int((codes < 0).sum())
    thin = (np.diff(off) < min_coverage) & (codes >= 0)
    codes[thin] = -1
    unlisted = np.zeros(len(codes), bool)
    if sites is not None:
        unlisted = ~_listed_rows(group, sites) & (codes >= 0)
        codes[unlisted] = -1
    sig = _encode(group['sig']) if len(codes) else np.zeros(0, np.int16)
    res = engine.kmer_mix_host(sig, off, codes, ncodes, mean0, sd0, model=mix_model, max_iter=max_iter, tol=tol, min_samples=2, device=device)
    kept = select_alt_codes(res, mean0, sd0, min_samples, min_pi, min_shift)
    st = res['status']
    log('kmer mix: k = %d, %d position(s) pooled over %d k-mer(s); %d k-mer(s) kept (n_used >= %d, pi >= %g, shift >= %g sd0), %d not '
        'converged, %d without a control entry; dropped: %d without a full k-mer, %d below MinCoverage%s'
        % (k, int(res['n_positions'].sum()), int((res['n_positions'] > 0).sum()), int(kept.sum()), int(min_samples), float(min_pi),
           float(min_shift), int(((st & L.KMIX_NOT_CONVERGED) != 0).sum()), int(((st & L.KMIX_NO_MODEL) != 0).sum()), no_context,
           int(thin.sum()), (', %d not among the sites' % int(unlisted.sum())) if sites is not None else ''))
    table = dict({f: res[f] for f in L.KMIX_COUNT_FIELDS + L.KMIX_FIELDS + ('iters', 'status')}, mean0=mean0, sd0=sd0, kept=kept)
    return alt_model_from(model, res, kept), table


def write_kmer_mix_table(path, model, table):
    """<FileID>_kmer_mix.txt: per k-mer the KMER_MIX_COLUMNS 'kmer n_positions n_used n_outside mean0 sd0 pi mu_mod sd_mod llr iters
    status kept' as '%s %d %d %d' + five '%.6f' + '%.3f %d %d %d' (Python's spelling of nan)"""
    k = int(model['k'])
    cols = [np.asarray(table[f]).tolist() for f in KMER_MIX_COLUMNS[1:-1]] + [np.asarray(table['kept']).astype(int).tolist()]
    with open(path, 'w') as f:
        f.writelines('%s %d %d %d %.6f %.6f %.6f %.6f %.6f %.3f %d %d %d\n' % ((kmer_string(c, k),) + row) for c, row in enumerate(zip(*cols)))


def model_profile(model, group, min_positions=1):
    """The kind-'model' profile (onesample.make_profile) of the rows of `group` that the model predicts: those whose k-mer is
    complete and whose table entry rests on at least min_positions positions and has a finite sd > 0.  onesample.mtest1 and
    `detect1 --refProfile` take it as any other profile."""
    codes = group_codes(group, int(model['k']), int(model['center']))
    c = np.where(codes >= 0, codes, 0)
    mean, sd = np.asarray(model['mean'], dtype=np.float64)[c], np.asarray(model['sd'], dtype=np.float64)[c]
    with np.errstate(invalid='ignore'):
        keep = (codes >= 0) & (np.asarray(model['n_positions'])[c] >= min_positions) & np.isfinite(mean) & np.isfinite(sd) & (sd > 0.0)
    rows = np.flatnonzero(keep)
    return onesample.make_profile(np.asarray(group['chrom'])[rows], np.asarray(group['strand'])[rows], np.asarray(group['pos'])[rows],
                                  np.asarray(group['base'])[rows], mean[rows], sd[rows])
