"""One-sample detection against a stored control profile (K9; include/nanomod_hip.h: nmod_one_sample).

A *profile* is what a position of a read group is reduced to: its coverage n, mean and ddof = 0 standard deviation at full
float64 precision (`_meanstd.cvs` prints three decimals and no coverage, so it cannot serve).  Two kinds:

    'control'  built from a read group (`build_profile`, `cli profile`): carries n, the sample is tested against it with the
               Welch t of the two-sample test (from the statistics) and a KS test against N(mean, sd^2);
    'model'    an expected level and spread per position from elsewhere (a k-mer table, a pool of earlier runs): no n, the
               reference is taken as known (one-sample t).

    prof = build_profile(container.load_group('control.npz'), min_coverage=5)
    save_profile('control_profile.npz', prof)
    mtest1({'ds2': ['s'], 's': {'nmod_container': container.load_group('native.npz')}, 'nmod_profile': 'control_profile.npz',
            'MinCoverage': 5, 'neighborPvalues': 2, 'WeightsDif': 2.0, 'testMethod': 'stouffer', 'rankUse': 'pv',
            'SaveTest': 1, 'outFolder': 'out', 'FileID': 'run1'})

The arithmetic runs in the HIP library; there is no CPU fallback.
"""
from __future__ import annotations

import os
import time

import numpy as np

from . import _lib as L
from . import container, detect, engine

PROFILE_VERSION = 1
PROFILE_FIELDS = ('version', 'kind', 'chrom_names', 'chrom_id', 'strand', 'pos', 'base', 'n', 'mean', 'sd')


def _encode(sig):
    """detect.encode_signals for one group; large float64 vectors pass through (the device sorts them as 64-bit keys)"""
    sig = np.asarray(sig)
    if sig.dtype == np.float64 and sig.size <= detect.DEVICE_ENCODE_ABOVE:
        return detect.encode_signals(sig)
    if sig.dtype not in (np.float32, np.int16, np.float64):
        return detect.encode_signals(sig.astype(np.float64))
    return np.ascontiguousarray(sig)


def _sorted_rows(g, rows, cid):
    """`rows` of a per-position group in the reference's order: sorted (chrom, strand), ascending position"""
    from . import cli
    keys = cli._keys(g, cid)[rows]
    if len(keys) > 1 and not bool(np.all(keys[1:] > keys[:-1])):
        order = np.argsort(keys, kind='stable')
        rows, keys = rows[order], keys[order]
    return rows, keys


def make_profile(chrom, strand, pos, base, mean, sd, n=None):
    """A profile from per-position arrays (pos 0-based), put into the reference's order.  n given: kind 'control'; n None: kind
    'model', which has no `n`."""
    from . import cli
    chrom = np.asarray(chrom).astype(str)
    g = dict(strand=np.asarray(strand).astype(str), pos=np.asarray(pos, dtype=np.int64))
    names, (cid,) = cli._chrom_codes(chrom)
    rows, _ = _sorted_rows(g, np.arange(len(chrom), dtype=np.int64), cid)
    prof = dict(version=np.int32(PROFILE_VERSION), kind='control' if n is not None else 'model',
                chrom_names=np.array(names, dtype=str), chrom_id=cid[rows].astype(np.int32), strand=g['strand'][rows], pos=g['pos'][rows],
                base=np.asarray(base).astype(str)[rows], mean=np.asarray(mean, dtype=np.float64)[rows],
                sd=np.asarray(sd, dtype=np.float64)[rows])
    if n is not None:
        prof['n'] = np.asarray(n, dtype=np.int32)[rows]
    return prof


def profile_moments(sig, off, device=0):
    """(mean, sd with ddof = 0, status) of CSR rows from a K9 run against the dummy reference mu = 0, sd = 1: the moments a later
    run is tested against are the ones the device reports, no other code computes them"""
    npos = len(off) - 1
    res = engine.one_sample_host(_encode(sig), off, np.zeros(npos), np.ones(npos), method='ks', device=device)
    return res['mean'], res['std'], res['status']


def build_profile(group, min_coverage=5, device=0, log=print):
    """The control profile of one read group (a per-position container: chrom, strand, pos, base, off, sig): the positions with at
    least min_coverage reads as (chrom, strand, pos, base, n, mean, sd) in the reference's order.  Positions the device cannot
    reduce (beyond L.MAX_ONE reads, or with non-finite samples) are left out and counted."""
    from . import cli
    rows = np.flatnonzero(np.diff(group['off']) >= min_coverage)
    names, (cid,) = cli._chrom_codes(group['chrom'])
    rows, _ = _sorted_rows(group, rows, cid)
    sig, off = container.gather_rows(group['sig'], group['off'], rows)
    mean, sd, status = profile_moments(sig, off, device) if len(rows) else (np.zeros(0), np.zeros(0), np.zeros(0, np.uint8))
    ok = (status & (L.STATUS_TOO_LARGE | L.STATUS_NONFINITE | L.STATUS_EMPTY)) == 0
    if not bool(np.all(ok)):
        log('profile: %d position(s) left out (beyond %d reads, or non-finite samples)' % (int((~ok).sum()), L.MAX_ONE))
    rows, mean, sd, n = rows[ok], mean[ok], sd[ok], np.diff(off)[ok].astype(np.int32)
    return dict(version=np.int32(PROFILE_VERSION), kind='control', chrom_names=np.array(names, dtype=str),
                chrom_id=cid[rows].astype(np.int32), strand=np.asarray(group['strand'])[rows].astype(str),
                pos=np.asarray(group['pos'], dtype=np.int64)[rows], base=np.asarray(group['base'])[rows].astype(str), n=n, mean=mean, sd=sd)


def save_profile(path, prof):
    """A profile as an uncompressed .npz (PROFILE_FIELDS; a model has no `n`); numpy appends '.npz' to a path without it."""
    arrays = {k: np.asarray(prof[k]) for k in PROFILE_FIELDS if k in prof}
    if (prof['kind'] == 'model') != ('n' not in arrays):
        raise ValueError("a 'control' profile needs n, a 'model' has none")
    np.savez(path, **arrays)


def load_profile(path):
    with np.load(path) as z:
        prof = {k: z[k] for k in PROFILE_FIELDS if k in z.files}
    prof['kind'] = str(prof['kind'])
    if int(prof['version']) != PROFILE_VERSION or prof['kind'] not in ('control', 'model'):
        raise ValueError('%s: not a version-%d profile' % (path, PROFILE_VERSION))
    m = len(prof['pos'])
    if (prof['kind'] == 'model') != ('n' not in prof) or any(len(prof[k]) != m for k in ('chrom_id', 'strand', 'base', 'mean', 'sd')):
        raise ValueError('%s: inconsistent profile' % path)
    return prof


def match_positions(group, prof, min_coverage, log=print):
    """The positions to test: those the sample group holds with at least min_coverage reads AND the profile holds (a control
    profile: with n >= min_coverage), in the reference's order.  Prints how many positions of either side were dropped.
    Returns (meta, sig, off, ref_mean, ref_sd, ref_n or None, run_id); meta['n1'] is the profile's n (0 for a model)."""
    from . import cli
    pchrom = np.asarray(prof['chrom_names']).astype(str)[np.asarray(prof['chrom_id'], dtype=np.int64)] if len(prof['pos']) else np.zeros(0, dtype=str)
    names, (cid_g, cid_p) = cli._chrom_codes(group['chrom'], pchrom)
    rows_g = np.flatnonzero(np.diff(group['off']) >= min_coverage)
    rows_g, kg = _sorted_rows(group, rows_g, cid_g)
    pg = dict(strand=np.asarray(prof['strand']), pos=np.asarray(prof['pos'], dtype=np.int64))
    rows_p = np.arange(len(pg['pos']), dtype=np.int64)
    if prof['kind'] == 'control':
        rows_p = rows_p[np.asarray(prof['n'])[rows_p] >= min_coverage]
    rows_p, kp = _sorted_rows(pg, rows_p, cid_p)
    common, ig, ip = np.intersect1d(kg, kp, assume_unique=True, return_indices=True)
    log('one-sample: %d position(s) tested; %d of the sample group dropped (%d below MinCoverage, %d not in the profile); '
        '%d of the profile dropped (%d below MinCoverage, %d not in the sample group)'
        % (len(common), len(group['pos']) - len(common), len(group['pos']) - len(rows_g), len(rows_g) - len(common),
           len(pg['pos']) - len(common), len(pg['pos']) - len(rows_p), len(rows_p) - len(common)))
    rg, rp = rows_g[ig], rows_p[ip]
    sig, off = container.gather_rows(group['sig'], group['off'], rg)
    sig = _encode(sig) if len(rg) else np.zeros(0, np.float32)
    chrom = np.asarray(group['chrom'])[rg]; strand = np.asarray(group['strand'])[rg]; pos = np.asarray(group['pos'], dtype=np.int64)[rg]
    ref_n = np.asarray(prof['n'], dtype=np.int32)[rp] if prof['kind'] == 'control' else None
    meta = dict(chrom=chrom, strand=strand, pos=pos, base=np.asarray(prof['base'])[rp], n0=np.diff(off).astype(np.int32),
                n1=ref_n if ref_n is not None else np.zeros(len(rg), np.int32), names=names, chrom_id=cid_g[rg].astype(np.int32))
    rid = detect.run_ids(chrom, strand, pos)
    return (meta, sig, off, np.asarray(prof['mean'], dtype=np.float64)[rp], np.asarray(prof['sd'], dtype=np.float64)[rp], ref_n, rid)


ONE_FDR_TRACKS = tuple(pq for pq in detect.FDR_TRACKS if pq[0] != 'mwu_p')


def one_fdr_tracks(res, with_comb, method, alpha=0.05, device=0):
    """detect.fdr_tracks for a one-sample result: q-values of t_p, ks_p and (iff with_comb) comb_p, one family per track"""
    pairs = [pq for pq in ONE_FDR_TRACKS if pq[0] != 'comb_p' or with_comb]
    qs, summ = engine.fdr_adjust_host([res[p] for p, _ in pairs], method=method, alpha=alpha, device=device)
    return {q: a for (_, q), a in zip(pairs, qs)}, {p: s for (p, _), s in zip(pairs, summ)}


def write_one_sample(path, meta, res, with_comb):
    """<FileID>_one_sample.txt: per position 'chrom strand pos+1 base n nref shift t pt D pKS' as '%s %s %d %s %d %d %.3f %.3f
    %.3E %.3f %.3E', then ' %.3f %.3E' with the combined pair iff with_comb: the number formats of _sign_test.txt (Python's
    spelling of nan / inf); nref is 0 for a model."""
    names = [str(n) for n in meta['names']]
    chrom = [names[i] for i in np.asarray(meta['chrom_id']).tolist()]
    strand, base = (list(engine._first_chars(meta[k]).decode()) for k in ('strand', 'base'))
    pos = (np.asarray(meta['pos'], dtype=np.int64) + 1).tolist()
    cols = [np.asarray(meta['n0']).tolist(), np.asarray(meta['n1']).tolist()]
    cols += [np.asarray(res[k], dtype=np.float64).tolist() for k in ('shift', 't_t', 't_p', 'ks_d', 'ks_p') + (('comb_st', 'comb_p') if with_comb else ())]
    fmt = '%s %s %d %s %d %d %.3f %.3f %.3E %.3f %.3E' + (' %.3f %.3E' if with_comb else '') + '\n'
    with open(path, 'w') as f:
        f.writelines(fmt % ((c, s, p, b) + row) for c, s, p, b, row in zip(chrom, strand, pos, base, zip(*cols)))


def _group_of(moptions):
    ds = moptions[moptions['ds2'][0]]
    return ds['nmod_container'] if 'nmod_container' in ds else container.from_moptions_dataset(ds)


def mtest1(moptions):
    """detect.mtest2 for ONE read group against a profile.  moptions keys read: 'ds2' (its first dataset: 'nmod_container' arrays or
    the reference's dicts), 'nmod_profile' (a profile dict or the path of one), 'MinCoverage', 'neighborPvalues', 'WeightsDif',
    'testMethod', 'rankUse', 'SaveTest', 'outFolder', 'FileID', 'outLevel', 'nmod_device', 'nmod_fdr' / 'nmod_fdr_alpha'.  Written:
    'one_sample_arrays' (engine.one_sample_host's dict), 'one_sample_meta', 'sorted_one_sample' (the ranked order, as indices),
    with nmod_fdr 'one_sample_fdr' ('t_q', 'ks_q', 'comb_q') and 'nmod_fdr_summary'; with SaveTest <FileID>_one_sample.txt and
    <FileID>_one_sample_fdr.txt."""
    dev = moptions.get('nmod_device', 0)
    engine.warm_up(dev)
    quiet = moptions.get('outLevel', detect.OUTPUT_ERROR) > detect.OUTPUT_ERROR
    log = (lambda *a: None) if quiet else print
    prof = moptions['nmod_profile']
    if isinstance(prof, (str, os.PathLike)):
        prof = load_profile(prof)
    meta, sig, off, mu, sd, ref_n, rid = match_positions(_group_of(moptions), prof, moptions['MinCoverage'], log)
    npos = len(rid)
    method, nb = moptions['testMethod'], moptions['neighborPvalues']
    if method not in ('ks', 'stouffer', 'fisher'):
        raise ValueError("testMethod must be 'ks', 'stouffer' or 'fisher', not %r" % (method,))
    start_time = time.time()
    with_comb = method != 'ks' and nb >= 0
    res = engine.one_sample_host(sig, off, mu, sd, ref_n, rid, nb=max(nb, 0), weights_dif=moptions.get('WeightsDif', 2.0),
                                 method=method if with_comb else 'ks', device=dev)
    flagged = np.flatnonzero(res['status'] & (L.STATUS_TOO_LARGE | L.STATUS_NONFINITE | L.STATUS_BAD_REFERENCE)) if npos else np.zeros(0, np.int64)
    moptions['nmod_flagged'] = [(str(meta['chrom'][i]), str(meta['strand'][i]), int(meta['pos'][i]), int(res['status'][i])) for i in flagged]
    if len(flagged):
        log('nanomod_amd: %d position(s) could not be tested (beyond %d reads, non-finite samples or an unusable reference) and carry '
            'NaN statistics; first: %r' % (len(flagged), L.MAX_ONE, moptions['nmod_flagged'][0]))
    fdr_method = detect._fdr_option(moptions)
    if fdr_method:
        moptions['one_sample_fdr'], moptions['nmod_fdr_summary'] = one_fdr_tracks(res, with_comb, fdr_method, float(moptions.get('nmod_fdr_alpha', 0.05)), dev)
    moptions['one_sample_arrays'] = res
    moptions['one_sample_meta'] = meta
    if moptions.get('outLevel', detect.OUTPUT_ERROR) <= detect.OUTPUT_INFO:
        print('Producing pvalues: consuming time %d' % (time.time() - start_time))
    if moptions.get('SaveTest', 0):
        os.makedirs(moptions['outFolder'], exist_ok=True)
        path = os.path.join(moptions['outFolder'], moptions['FileID'] + '_one_sample.txt')
        write_one_sample(path, meta, res, with_comb and nb > 0)
        log('Test data is saved in', path)
        if fdr_method:
            detect.write_sign_test_fdr(os.path.join(moptions['outFolder'], moptions['FileID'] + '_one_sample_fdr.txt'), meta, moptions['one_sample_fdr'])
    pv = moptions.get('rankUse', 'pv') == 'pv'
    ks_key = res['ks_p' if pv else 'ks_d']
    first = res['comb_p' if pv else 'comb_st'] if with_comb else ks_key
    t_key = res['t_p'] if pv else np.abs(res['t_t'])
    moptions['sorted_one_sample'] = engine.rank_order_host(first, ks_key, t_key, descending=not pv, device=dev) if npos else np.zeros(0, np.int32)
    return moptions['sorted_one_sample']
