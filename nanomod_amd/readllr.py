"""Per-read calls by the log-likelihood ratio between two k-mer models (K13; include/nanomod_hip.h: nmod_read_llr,
nmod_site_llr).

`readcalls` scores every event against the unmodified model alone: an outlier test.  With a second table, built by `kmermodel` from a
fully modified control, every event has a log-likelihood ratio ln N(x; modified) - ln N(x; unmodified); summed over the events of the
same read whose k-mer covers a base it says which of the two levels the read shows there: modified (the sum is at least `thr`),
canonical (at most -thr) or neither.  Per position, the modified share of the reads that are one or the other.

    canonical, modified = (kmermodel.load_kmer_model(p) for p in ('control_kmer_model.npz', 'modified_kmer_model.npz'))
    table, sites = call_reads_llr(container.load_reads('sample_reads.npz'), canonical, modified, rescale=dict(min_events=50))
    write_read_llr('run_read_llr.txt', table); write_site_llr('run_site_llr.txt', sites)

The rescaling (K11, against the unmodified model), the ratios, the grouping by position and the counts all run in the HIP library on
the device, one after the other on one stream; there is no CPU fallback.

compare_reads_llr compares the modified share of every site between two samples (K15); cooccur_reads_llr keeps the read and asks of every
pair of nearby candidate sites whether they are modified on the same molecules (K16, nmod_site_pairs): a 2 x 2 table of the reads
called at both sites, its log odds ratio, phi and the exact test.
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib as L
from . import engine
from . import rescale as _rescale
from . import tables as T
from .sitemod import moderated_entry, write_site_diff_mod         # (K25: the moderated chain step and the writer of its two files)
from .multimod import call_reads_llr_multi, write_read_llr_multi, write_site_llr_multi, write_site_compose   # (K26: several modified tables at once)
from .readcalls import _RESCALE_KEYS, _checked_reads, _known_options, _open_device, _pivot_sites, _read_table, _upload_rescaled


_STOICH_KEYS = ('min_valid', 'ci_level', 'max_iter', 'tol')


def _llr_setup(model, alt_model, window, thr, prior, min_positions, rescale):
    """The two masked models and K13's options of the entries that score a read-level set, with their refusals, before any device
    work: (m0, m1, k, center, prior_logit, opts)"""
    m0 = _rescale.masked_model(model, min_positions)
    m1 = _rescale.masked_model(alt_model, min_positions)
    k, center = m0['k'], m0['center']
    if (m1['k'], m1['center']) != (k, center):
        raise ValueError('the two models must share k and center: %d / %d and %d / %d' % (k, center, m1['k'], m1['center']))
    prior = float(prior)
    if not 0.0 < prior < 1.0:
        raise ValueError('prior must lie inside (0, 1)')
    prior_logit = math.log(prior / (1.0 - prior))
    _known_options('rescale', rescale, _RESCALE_KEYS)
    opts, _ = engine._llr_opts(window, thr, prior_logit, k, center, k, center, ())           # the refusals, before any device work
    return m0, m1, k, center, prior_logit, opts


def _scorer(setup, rescale, thr, device):
    """Open the device and upload the two models once: (det, t, score).  score(sample, want) uploads one checked sample (val, off, base),
    rescales it against the unmodified model when `rescale` is a dict (K11) and scores it with K13: (d_off, nmod_read_llr's results
    with the event tracks `want`, the rescale fit or None)"""
    m0, m1, k, center, prior_logit, opts = setup
    det, t = _open_device(device)
    d_models = t(m0['mean']), t(m0['sd']), t(m1['mean']), t(m1['sd'])

    def score(sample, want=('llr_win',)):
        d_val, d_off, d_base, fit = _upload_rescaled(det, t, sample, d_models[0], d_models[1], k, center, rescale)
        calls = det.read_llr(d_val, d_off, d_base, *d_models, k, center, window=(opts.nb_lo, opts.nb_hi), thr=thr, prior_logit=prior_logit,
                             want=want)
        return d_off, calls, fit
    return det, t, score


def call_reads_llr(reads, model, alt_model, *, window='kmer', thr=2.5, prior=0.5, min_positions=1, rescale=None, events=False, device=0,
                   log=print, stoich=None):
    """Call the events of a read-level set (container.READ_FIELDS) between an unmodified and a modified k-mer model
    (kmermodel.KMER_MODEL_FIELDS, one k and center).  window: 'kmer' (the events whose k-mer holds the base) or (lo, hi) events of the
    same read before and after; thr: the window sum from which an event is called; prior: the prior probability of the modified state
    behind the posterior track p_mod (it does not move the calls).  rescale: None, or a dict of rescale.rescale_reads' fit options: the
    reads are first put on the unmodified model's scale on the device.
    Returns (table, sites) — and with `events` a third dict of the per-event tracks llr, llr_win, p_mod (float64, in the reads' layout):
    table: one entry per read: index, chrom, strand, start, events, n_sites (scored events), n_mod, n_can, status (L.CALLS_TOO_LARGE)
      and, when rescaled, shift, scale, rescale_status;
    sites: one entry per covered position in the reference's row order: chrom, strand, pos, base, n_reads (the events there), n_valid
      (the scored ones), n_mod, n_can, frac = n_mod / (n_mod + n_can) (NaN without a confident read).
    stoich: None, or a dict of engine.site_stoich_host's options (min_valid, ci_level, max_iter, tol; {} for the defaults): the
      modified share of every position by maximum likelihood over all its window sums (K14, nmod_site_stoich) on the same stream;
      `sites` gains pi, pi_lo, pi_hi, stat, p_null (float64), iters (int32) and stoich_status (uint8, L.STOICH_* bits).
    One summary line goes to `log`."""
    setup = _llr_setup(model, alt_model, window, thr, prior, min_positions, rescale)
    opts = setup[-1]
    if stoich is not None:
        _known_options('stoich', stoich, _STOICH_KEYS)
        engine._stoich_opts(*(stoich.get(key, default) for key, default in zip(_STOICH_KEYS, (3, 0.95, 60, 1e-12))))
    val, off, base = _checked_reads(reads, 'reads')
    nreads = len(off) - 1
    det, _, score = _scorer(setup, rescale, thr, device)
    _, calls, fit = score((val, off, base), L.LLR_EVENT_FIELDS if events else ('llr_win',))
    piv = engine.pivot_reads(reads, device, val=calls['llr_win'])
    counts = det.site_llr(piv['sig'], off=piv['off'], thr=thr)
    share = det.site_stoich(piv['sig'], off=piv['off'], **stoich) if stoich is not None else None

    table = _read_table(reads, off, calls, L.LLR_READ_FIELDS, fit)
    sites = _pivot_sites(piv, counts, L.SITE_LLR_FIELDS)
    clause = ''
    if share is not None:
        sites.update({f: share[f].cpu().numpy() for f in L.STOICH_FIELDS + ('iters',)}, stoich_status=share['status'].cpu().numpy())
        clause = '; %d position(s) with a modified share, %d of them with an interval above 0' % (
            int(((sites['stoich_status'] & L.STOICH_NO_ESTIMATE) == 0).sum()), int((sites['pi_lo'] > 0.0).sum()))
    log('readllr: %d read(s), %d of %d event(s) scored, %d modified and %d canonical at threshold %g over %d + 1 + %d event(s); '
        '%d position(s), %d with a modified call%s%s'
        % (nreads, int(table['n_sites'].sum()), len(val), int(table['n_mod'].sum()), int(table['n_can'].sum()), float(thr), opts.nb_lo, opts.nb_hi,
           len(sites['pos']), int((sites['n_mod'] > 0).sum()),
           '' if fit is None else '; %d read(s) not rescaled' % int(((table['rescale_status'] & L.RESCALE_FAILED) != 0).sum()), clause))
    if events:
        return table, sites, {f: calls[f].cpu().numpy() for f in L.LLR_EVENT_FIELDS}
    return table, sites


def write_read_llr(path, table):
    """<FileID>_read_llr.txt: per read 'index chrom strand start events n_sites n_mod n_can status' as '%d %s %s %d %d %d %d %d %d'"""
    T.write_rows(path, '%d %s %s %d %d %d %d %d %d\n', T.read_cols(table) + T.fields(table, 'start', 'events', 'n_sites', 'n_mod', 'n_can', 'status'))


def write_site_llr(path, sites):
    """<FileID>_site_llr.txt: per position 'chrom strand pos+1 base n_reads n_valid n_mod n_can frac' as '%s %s %d %s %d %d %d %d %.6f'
    (the position 1-based like every text output; frac 'nan' where no read is confident)"""
    T.write_rows(path, '%s %s %d %s %d %d %d %d %.6f\n',
                 T.site_cols(sites, base=True) + T.fields(sites, 'n_reads', 'n_valid', 'n_mod', 'n_can', 'frac'))


def write_site_stoich(path, sites):
    """<FileID>_site_stoich.txt: per position 'chrom strand pos+1 base n_reads n_valid pi pi_lo pi_hi stat p_null status' as
    '%s %s %d %s %d %d %.6f %.6f %.6f %.3f %.3E %d' (the position 1-based; 'nan' as Python spells it where the position has no
    estimate; `sites` of call_reads_llr(..., stoich=...))"""
    T.write_rows(path, '%s %s %d %s %d %d %.6f %.6f %.6f %.3f %s %d\n',
                 T.site_cols(sites, base=True) + T.fields(sites, 'n_reads', 'n_valid', 'pi', 'pi_lo', 'pi_hi', 'stat') + [T.sci(sites['p_null'])] +
                 T.fields(sites, 'stoich_status'))


_DIFF_KEYS = ('min_valid', 'ci_level', 'max_iter', 'tol')
SITE_DIFF_FIELDS = ('pi0', 'pi1', 'pi_pool', 'delta', 'delta_lo', 'delta_hi', 'stat', 'p_diff')
_REP_KEYS = ('min_valid', 'ci_level', 'phi_floor', 'max_iter', 'tol')
SITE_DIFF_REP_FIELDS = ('pi0', 'pi1', 'pi_pool', 'delta', 'delta_lo', 'delta_hi', 'stat_cond', 'p_cond', 'stat_het', 'p_het', 'phi', 'p_rep')

# What follows the per-sample chain in the two comparisons: the options of `diff` and their check, the matcher of the pivots' rows, the
# entry, the columns between `base` and the entry's float fields, the p-value track that goes to fdr, the status key and its no-estimate
# bit, and the words of the names refusal and of the summary line.
_TWO_SAMPLES = dict(
    keys=_DIFF_KEYS, defaults=(3, 0.95, 60, 1e-12), check=lambda G, n_control, *v: engine._diff_opts(*v),
    match=lambda pivots, n_control, min_coverage, device: engine.match_score_rows(pivots[0], pivots[1], min_coverage, device),
    entry=lambda det, rows, G, n_control, diff: det.site_diff(rows['sig0'], rows['sig1'], off0=rows['off0'], off1=rows['off1'], **diff),
    columns=lambda rows, res, G, n_control: dict(
        n_reads0=np.diff(rows['off0'].cpu().numpy()).astype(np.int32), n_reads1=np.diff(rows['off1'].cpu().numpy()).astype(np.int32),
        n_valid0=res['n_valid0'].cpu().numpy(), n_valid1=res['n_valid1'].cpu().numpy()),
    fields=SITE_DIFF_FIELDS, track='p_diff', status='diff_status', no_estimate=L.DIFF_NO_ESTIMATE, whose='both samples',
    summary=lambda nreads, n_control: 'readdiff: %d and %d read(s); %%d site(s) in both samples' % tuple(nreads))
_REPLICATED = dict(
    keys=_REP_KEYS, defaults=(3, 0.95, 0.0, 60, 1e-12), check=lambda G, n_control, *v: engine._rep_opts(G, n_control, *v),
    match=lambda pivots, n_control, min_coverage, device: engine.match_score_rows_multi(pivots, n_control, min_coverage, device),
    entry=lambda det, rows, G, n_control, diff: det.site_diff_rep(rows['sig'], rows['off'], G, n_control, **diff),
    columns=lambda rows, res, G, n_control: dict(n_samples=G, n_control=n_control, n_valid=res['n_valid'].cpu().numpy().reshape(-1, G),
                                                 pi_s=res['pi_s'].cpu().numpy().reshape(-1, G)),
    fields=SITE_DIFF_REP_FIELDS, track='p_rep', status='rep_status', no_estimate=L.REP_NO_ESTIMATE, whose='all samples',
    summary=lambda nreads, n_control: 'readdiff: %d and %d sample(s) of %s read(s); %%d site(s) in every sample'
                                      % (n_control, len(nreads) - n_control, ', '.join(str(n) for n in nreads)))


_MODERATED = dict(_REPLICATED, entry=moderated_entry, fields=SITE_DIFF_REP_FIELDS + ('phi_post', 'rep_prior'))


def _compare(tail, reads, labels, n_control, model, alt_model, window, thr, prior, min_positions, rescale, min_coverage, diff, fdr, fdr_alpha,
             names, device, log):
    """compare_reads_llr and compare_reads_llr_rep: the chain of every sample of `reads` (labelled `labels` in a refusal), the first
    n_control of them the control condition's, then the `tail` (_TWO_SAMPLES or _REPLICATED)"""
    G = len(reads)
    setup = _llr_setup(model, alt_model, window, thr, prior, min_positions, rescale)
    _known_options('diff', diff, tail['keys'])
    tail['check'](G, n_control, *(diff.get(key, default) for key, default in zip(tail['keys'], tail['defaults'])))
    if fdr is not None:
        engine._fdr_method(fdr)
    if int(min_coverage) != min_coverage or int(min_coverage) < 1:
        raise ValueError('min_coverage must be an integer >= 1, not %r' % (min_coverage,))
    samples = [_checked_reads(r, label) for r, label in zip(reads, labels)]
    every = engine.chrom_names(*reads)
    names = every if names is None else [str(n) for n in names]
    lacking = sorted(set(every) - set(names))
    if lacking or names != sorted(set(names)):
        raise ValueError('names must be the sorted chromosome names of %s; missing or out of order: %s' % (tail['whose'], ', '.join(lacking) or 'order'))
    det, _, score = _scorer(setup, rescale, thr, device)
    pivots = [engine.pivot_reads(r, device, names=names, val=score(sample)[1]['llr_win']) for r, sample in zip(reads, samples)]
    rows = tail['match'](pivots, n_control, int(min_coverage), device)
    res = tail['entry'](det, rows, G, n_control, diff)
    q = None
    if fdr is not None:
        (q,), _ = det.fdr(res, tracks=(tail['track'],), method=fdr, alpha=fdr_alpha)
    sites = dict(engine.key_sites(rows['key'].cpu().numpy(), names), base=rows['base'].cpu().numpy().view('S1').astype('U1'),
                 **tail['columns'](rows, res, G, n_control), **{f: res[f].cpu().numpy() for f in tail['fields']})
    if q is not None:
        sites['q'] = q.cpu().numpy()
    status = sites[tail['status']] = res['status'].cpu().numpy()
    est = (status & tail['no_estimate']) == 0
    log((tail['summary']([len(s[1]) - 1 for s in samples], n_control) +
         ' with at least %d read(s), %d with an estimate, %d with an interval of delta that excludes 0%s')
        % (len(sites['pos']), int(min_coverage), int(est.sum()), int((est & ((sites['delta_lo'] > 0.0) | (sites['delta_hi'] < 0.0))).sum()),
           '' if q is None else '; %d with q <= %g (%s)' % (int((sites['q'] <= fdr_alpha).sum()), fdr_alpha, fdr)))
    return sites


def compare_reads_llr(reads0, reads1, model, alt_model, *, window='kmer', thr=2.5, prior=0.5, min_positions=1, rescale=None,
                      min_coverage=1, diff={}, fdr=None, fdr_alpha=0.05, names=None, device=0, log=print):
    """Compare the modified share of every site between two read-level sets (container.READ_FIELDS): reads0 the control condition,
    reads1 the other.  Per sample the optional rescaling (K11) and the window sums (K13) as in call_reads_llr; both are grouped by
    position with one list of chromosome names, the sites both hold with at least min_coverage reads are matched
    (engine.match_score_rows) and compared by nmod_site_diff (K15), all on the device and on one stream.  diff: a dict of
    engine.site_diff_host's options (min_valid, ci_level, max_iter, tol; {} for the defaults).  fdr: None, 'bh' or 'by': p_diff goes
    through nmod_fdr_adjust on the device at fdr_alpha and `sites` gains q.  names: the chromosome names both pivots use (default:
    those of both sets together; a list that lacks one of them is refused).
    Returns `sites`, one entry per matched site in the reference's row order: chrom, strand, pos, base, n_reads0, n_reads1, n_valid0,
    n_valid1, pi0, pi1, pi_pool, delta, delta_lo, delta_hi, stat, p_diff, [q,] diff_status (uint8, L.DIFF_* bits).  One summary line
    goes to `log`."""
    return _compare(_TWO_SAMPLES, [reads0, reads1], ['reads0', 'reads1'], 1, model, alt_model, window, thr, prior, min_positions, rescale,
                    min_coverage, diff, fdr, fdr_alpha, names, device, log)


def write_site_diff(path, sites):
    """<FileID>_site_diff.txt: per site 'chrom strand pos+1 base n_reads0 n_reads1 n_valid0 n_valid1 pi0 pi1 pi_pool delta delta_lo
    delta_hi stat p_diff [q] status' as '%s %s %d %s %d %d %d %d' + six '%.6f' + '%.3f %.3E [%.3E] %d' (the position 1-based; 'nan' as
    Python spells it where the site has no estimate; `sites` of compare_reads_llr)"""
    q_cols, q_fmt = T.sci_if(sites, 'q')
    T.write_rows(path, '%s %s %d %s %d %d %d %d %.6f %.6f %.6f %.6f %.6f %.6f %.3f %s ' + q_fmt + '%d\n',
                 T.site_cols(sites, base=True) + T.fields(sites, 'n_reads0', 'n_reads1', 'n_valid0', 'n_valid1', 'pi0', 'pi1', 'pi_pool', 'delta',
                                                          'delta_lo', 'delta_hi', 'stat') + [T.sci(sites['p_diff'])] + q_cols +
                 T.fields(sites, 'diff_status'))


def compare_reads_llr_rep(reads0_list, reads1_list, model, alt_model, *, window='kmer', thr=2.5, prior=0.5, min_positions=1, rescale=None,
                          min_coverage=1, diff={}, fdr=None, fdr_alpha=0.05, names=None, device=0, log=print, moderate=False):
    """Compare the modified share of every site between two replicated conditions: reads0_list the read-level sets
    (container.READ_FIELDS) of the control condition's replicates, reads1_list those of the other; three or more sets in all.
    compare_reads_llr's chain per sample — the optional rescaling (K11), the window sums (K13), the pivot with one list of chromosome
    names — then the sites every sample holds with at least min_coverage reads (engine.match_score_rows_multi) compared by
    nmod_site_diff_rep (K24).  diff: a dict of engine.site_diff_rep_host's options (min_valid, ci_level, phi_floor, max_iter, tol).
    fdr: None, 'bh' or 'by': p_rep goes through nmod_fdr_adjust on the device at fdr_alpha and `sites` gains q.
    Returns `sites`, one entry per matched site: chrom, strand, pos, base, n_samples, n_control, n_valid and pi_s (npos x G), pi0, pi1,
    pi_pool, delta, delta_lo, delta_hi, stat_cond, p_cond, stat_het, p_het, phi, p_rep, [q,] rep_status (uint8, L.REP_* bits).  One
    summary line goes to `log`.
    moderate: shrink the dispersions across sites (K25): K24 without its interval for phi, nmod_rep_prior over all matched sites, then
    nmod_site_diff_rep_mod.  p_rep, the interval and q are then the moderated ones, and `sites` gains phi_post, df_tot and rep_prior (the
    record as a dict of L.REP_PRIOR_FIELDS); a second line about the prior goes to `log`.  The three fits run twice."""
    n0, n1 = len(reads0_list), len(reads1_list)
    sites = _compare(_MODERATED if moderate else _REPLICATED, list(reads0_list) + list(reads1_list),
                     ['reads0[%d]' % i for i in range(n0)] + ['reads1[%d]' % i for i in range(n1)],
                     n0, model, alt_model, window, thr, prior, min_positions, rescale, min_coverage, diff, fdr, fdr_alpha, names, device, log)
    if moderate:
        rec = sites['rep_prior'] = dict(zip(L.REP_PRIOR_FIELDS, sites['rep_prior'].tolist()))
        sites['df_tot'] = rec['df_tot']
        log('readdiff: the prior of the dispersions rests on %d site(s) (%d more at 0): d0 %g, s0^2 %g; p_rep on %g degrees of freedom'
            % (int(rec['n_used']), int(rec['n_zero']), rec['d0'], rec['s0sq'], rec['df_tot']))
    return sites


def write_site_diff_rep(path, sites):
    """<FileID>_site_diff_rep.txt: per site 'chrom strand pos+1 base G', then n_valid and pi_s of every sample ('%d %.6f' each), then
    'pi0 pi1 pi_pool delta delta_lo delta_hi stat_cond p_cond stat_het p_het phi p_rep [q] status' as six '%.6f' + '%.3f %.3E %.3f
    %.3E %.3f %.3E [%.3E] %d' (write_site_diff's formats: the position 1-based; 'nan' as Python spells it where the site has no
    estimate; `sites` of compare_reads_llr_rep)"""
    G = int(sites['n_samples'])
    nv, ps = np.asarray(sites['n_valid']).reshape(-1, G), np.asarray(sites['pi_s']).reshape(-1, G)
    per = [col.tolist() for g in range(G) for col in (nv[:, g], ps[:, g])]
    q_cols, q_fmt = T.sci_if(sites, 'q')
    T.write_rows(path, '%s %s %d %s %d ' + '%d %.6f ' * G + '%.6f %.6f %.6f %.6f %.6f %.6f %.3f %s %.3f %s %.3f %s ' + q_fmt + '%d\n',
                 T.site_cols(sites, base=True) + [[G] * len(nv)] + per +
                 T.fields(sites, 'pi0', 'pi1', 'pi_pool', 'delta', 'delta_lo', 'delta_hi', 'stat_cond') +
                 [T.sci(sites['p_cond'])] + T.fields(sites, 'stat_het') + [T.sci(sites['p_het'])] + T.fields(sites, 'phi') + [T.sci(sites['p_rep'])] +
                 q_cols + T.fields(sites, 'rep_status'))


_PAIR_STAT_FIELDS = ('log_or', 'se', 'phi', 'p_fisher')
LINK_MIN_READS = 20         # reads valid at both sites below which the soft linkage of a pair is not fitted (include/nanomod_hip.h, K18)


def read_sites_file(path):
    """A list of candidate sites: lines 'chrom strand pos' with 1-based positions; further columns are ignored, so the first three of
    <FileID>_site_stoich.txt work, and so do empty lines and lines that start with '#'.  Returns (chrom, strand, pos) arrays, pos
    0-based."""
    chrom, strand, pos = [], [], []
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            parts = line.split()
            if not parts or parts[0].startswith('#'):
                continue
            if len(parts) < 3 or parts[1] not in ('+', '-') or not parts[2].isdigit() or int(parts[2]) < 1:
                raise ValueError("%s, line %d: expected 'chrom strand pos' with strand + or - and a 1-based position" % (path, ln))
            chrom.append(parts[0]); strand.append(parts[1]); pos.append(int(parts[2]) - 1)
    return np.array(chrom, dtype=str), np.array(strand, dtype=str).astype('U1'), np.array(pos, dtype=np.int64)


def site_keys(sites, names):
    """(chrom, strand, pos) arrays as nmod_pivot_reads' keys cs << 40 | pos over the chromosome list `names`: sorted, duplicates
    dropped; a site on a chromosome outside `names` can be covered by no read and is dropped too"""
    chrom, strand, pos = (np.asarray(x) for x in sites)
    chrom, strand, pos = chrom.astype(str), strand.astype(str), pos.astype(np.int64)
    if not (len(chrom) == len(strand) == len(pos)):
        raise ValueError('sites: chrom, strand and pos need one entry per site')
    if len(pos) and (pos.min() < 0 or pos.max() >= 1 << 40):
        raise ValueError('sites: positions must lie in 0 .. 2^40 - 1')
    known = np.isin(chrom, np.array(names, dtype=str)) if len(chrom) else np.zeros(0, bool)
    cs = engine.chrom_strand_ids(chrom[known], strand[known], names, 'sites').astype(np.int64)
    return np.unique((cs << 40) | pos[known])


def _sites_by_stoich(sites):
    by_stoich = isinstance(sites, str)
    if by_stoich and sites != 'stoich':
        raise ValueError("sites must be 'stoich' or (chrom, strand, pos) arrays")
    return by_stoich


def _site_scores(reads, setup, sites, site_alpha, rescale, thr, device, want_share=False):
    """The window sums (K13, after the optional rescaling K11) of a read-level set and the candidate sites, on the device and on one
    stream: sites 'stoich' (K14's estimates whose Benjamini-Hochberg q of p_null is at most site_alpha) or (chrom, strand, pos) arrays.
    Returns a dict: det, names, nreads, the CUDA vectors d_cs, d_start, d_off, llr_win and d_key, and with want_share site_pi: K14's
    estimates at the candidate sites that have one (a CUDA vector)."""
    import torch
    by_stoich = _sites_by_stoich(sites)
    sample = _checked_reads(reads, 'reads')
    nreads = len(sample[1]) - 1
    names = engine.chrom_names(reads)
    cs = engine.chrom_strand_ids(np.asarray(reads['chrom']).astype(str), np.asarray(reads['strand']).astype(str), names)
    start = np.ascontiguousarray(reads['start'], dtype=np.int64)
    host_key = None if by_stoich else site_keys(sites, names)
    det, t, score = _scorer(setup, rescale, thr, device)
    d_off, calls, _ = score(sample)
    llr_win = calls['llr_win']
    dev = llr_win.device
    site_pi = None
    if by_stoich or want_share:
        piv = engine.pivot_reads(reads, device, names=names, val=llr_win)
        share = det.site_stoich(piv['sig'], off=piv['off'])
        estimated = (share['status'] & L.STOICH_NO_ESTIMATE) == 0
    if by_stoich:
        (q_site,), _ = det.fdr(share, tracks=('p_null',), method='bh', alpha=site_alpha)
        keep = estimated & (q_site <= site_alpha)                                             # (a NaN q compares false)
        d_key = piv['key'][keep].contiguous()
    else:
        d_key = t(host_key)
        keep = (estimated & torch.isin(piv['key'], d_key)) if want_share else None
    if want_share:
        site_pi = share['pi'][keep]
    res = dict(det=det, names=names, nreads=nreads, d_cs=t(cs), d_start=t(start), d_off=d_off, llr_win=llr_win, d_key=d_key, site_pi=site_pi)
    if want_share == 'per_site':                  # K14's estimate of every candidate site in d_key's order, NaN where it has none
        pk = piv['key']                           # (and its count of scored reads, 0 at a site K14 has no row for)
        if pk.numel() == 0 or d_key.numel() == 0:
            res['site_pi_at'] = torch.full((d_key.numel(),), math.nan, dtype=torch.float64, device=dev)
            res['site_n_valid_at'] = torch.zeros(d_key.numel(), dtype=torch.int32, device=dev)
        else:
            at = torch.searchsorted(pk, d_key).clamp_(max=pk.numel() - 1)
            res['site_pi_at'] = torch.where((pk[at] == d_key) & estimated[at], share['pi'][at], torch.full_like(share['pi'][at], math.nan))
            res['site_n_valid_at'] = torch.where(pk[at] == d_key, share['n_valid'][at], torch.zeros_like(share['n_valid'][at]))
    return res


def cooccur_reads_llr(reads, model, alt_model, *, sites='stoich', max_dist=100, thr=2.5, min_reads=10, window='kmer', prior=0.5,
                      min_positions=1, rescale=None, fdr=None, fdr_alpha=0.05, site_alpha=0.05, device=0, log=print, soft=False,
                      ci_level=0.95):
    """Same-read co-occurrence of modification calls at pairs of sites of one read-level set (container.READ_FIELDS): are two sites
    modified on the same molecules?  The optional rescaling (K11) and the window sums (K13) as in call_reads_llr; then the candidate
    sites; then, read by read, the 2 x 2 table of every pair of candidate sites on one (chrom, strand) at most max_dist apart over the
    reads that have a call (modified: window sum >= thr, canonical: <= -thr) at both, with its log odds ratio, phi and two-sided exact
    test (K16, nmod_pair_index / nmod_site_pairs), all on the device and on one stream.
    sites: 'stoich': the positions to which nmod_site_stoich (K14) gives an estimate whose Benjamini-Hochberg q of p_null is at most
      site_alpha; or (chrom, strand, pos) arrays, pos 0-based (read_sites_file reads them from a text file).
    min_reads: reads with a call at both sites below which a pair gets no statistics.  fdr: None, 'bh' or 'by': p_fisher goes through
    nmod_fdr_adjust on the device at fdr_alpha and `pairs` gains q.
    Returns `pairs`, one entry per pair in key order: chrom, strand, pos_a, pos_b (0-based), dist, n11, n10, n01, n00 (the first index
    is site a's call), log_or, se, phi, p_fisher, [q,] status (uint8, L.PAIRS_* bits).  One summary line goes to `log`.
    soft: also the soft linkage of every pair from the window sums of all the reads that cover both sites with a valid sum, not only
      those beyond +-thr (K18, nmod_pair_rows_count / nmod_pair_rows_fill / nmod_pair_linkage, on the same stream): `pairs` gains n_cov
      (those reads), pa, pb (the marginal modified shares), d (the linkage) with its likelihood interval d_lo, d_hi at ci_level, r,
      pi11, pi10, pi01, pi00 (the cells of the joint law from pa, pb and d), stat, p_indep (the likelihood-ratio test of independence),
      link_status (uint8, L.LINK_* bits) and with fdr q_indep; a second line goes to `log`.  A pair needs max(min_reads, LINK_MIN_READS)
      such reads: below that the chi2 law of stat is liberal.  Without `soft` nothing changes."""
    setup = _llr_setup(model, alt_model, window, thr, prior, min_positions, rescale)
    engine._pairs_opts(thr, min_reads, False, ())
    link_min_reads = max(int(min_reads), LINK_MIN_READS)
    if soft:
        engine._link_opts(link_min_reads, ci_level, 60, 1e-12)
    max_dist = engine._check_max_dist(max_dist)
    if fdr is not None:
        engine._fdr_method(fdr)
    engine._check_alpha(fdr_alpha)
    site_alpha = engine._check_alpha(site_alpha)
    by_stoich = _sites_by_stoich(sites)
    sc = _site_scores(reads, setup, sites, site_alpha, rescale, thr, device)
    det, names, nreads, d_off, llr_win, d_key, d_cs, d_start = (sc[f] for f in ('det', 'names', 'nreads', 'd_off', 'llr_win', 'd_key', 'd_cs', 'd_start'))
    poff, npairs = det.pair_index(d_key, max_dist)
    res = det.site_pairs(d_cs, d_start, d_off, llr_win, d_key, poff, npairs, thr=thr, min_reads=min_reads)
    q = None
    if fdr is not None:
        (q,), _ = det.fdr(res, tracks=('p_fisher',), method=fdr, alpha=fdr_alpha)
    link = q_indep = None
    if soft:
        rows = det.pair_rows(d_cs, d_start, d_off, llr_win, d_key, poff, npairs)
        link = det.pair_linkage(rows['sa'], rows['sb'], rows['prow_off'], min_reads=link_min_reads, ci_level=ci_level)
        if fdr is not None:
            (q_indep,), _ = det.fdr(link, tracks=('p_indep',), method=fdr, alpha=fdr_alpha)
    key = d_key.cpu().numpy()
    first, second = res['first'].cpu().numpy().astype(np.int64), res['second'].cpu().numpy().astype(np.int64)
    counts = res['counts'].cpu().numpy().reshape(-1, 4)
    a, b = engine.key_sites(key[first], names), engine.key_sites(key[second], names)
    pairs = dict(chrom=a['chrom'], strand=a['strand'], pos_a=a['pos'], pos_b=b['pos'], dist=b['pos'] - a['pos'],
                 n11=counts[:, 3].copy(), n10=counts[:, 2].copy(), n01=counts[:, 1].copy(),
                 n00=counts[:, 0].copy(), **{f: res[f].cpu().numpy() for f in _PAIR_STAT_FIELDS})
    if q is not None:
        pairs['q'] = q.cpu().numpy()
    pairs['status'] = res['status'].cpu().numpy()
    tested = (pairs['status'] & L.PAIRS_TOO_FEW) == 0
    log('readpairs: %d read(s); %d candidate site(s)%s, %d pair(s) at most %d apart, %d with at least %d read(s) called at both sites%s'
        % (nreads, len(key), ' with q <= %g of the modified share' % site_alpha if by_stoich else '', npairs, max_dist, int(tested.sum()),
           int(min_reads), '' if q is None else '; %d with q <= %g (%s)' % (int((pairs['q'] <= fdr_alpha).sum()), fdr_alpha, fdr)))
    if link is not None:
        lk = {f: link[f].cpu().numpy() for f in L.LINK_FIELDS + ('n_valid', 'status')}
        pairs.update(n_cov=lk['n_valid'], **{f: lk[f] for f in ('pa', 'pb', 'd', 'd_lo', 'd_hi', 'r')})
        pa, pb, d = lk['pa'], lk['pb'], lk['d']
        pairs.update(pi11=pa * pb + d, pi10=pa * (1.0 - pb) - d, pi01=(1.0 - pa) * pb - d, pi00=(1.0 - pa) * (1.0 - pb) + d,
                     stat=lk['stat'], p_indep=lk['p_indep'], link_status=lk['status'])
        if q_indep is not None:
            pairs['q_indep'] = q_indep.cpu().numpy()
        fitted = (lk['status'] & L.LINK_NO_ESTIMATE) == 0
        log('readpairs: soft linkage of %d pair(s) with at least %d read(s) valid at both sites%s'
            % (int(fitted.sum()), link_min_reads,
               '' if q_indep is None else '; %d with q_indep <= %g (%s)' % (int((pairs['q_indep'] <= fdr_alpha).sum()), fdr_alpha, fdr)))
    return pairs


def write_site_pairs(path, pairs):
    """<FileID>_site_pairs.txt: per pair 'chrom strand pos_a+1 pos_b+1 dist n11 n10 n01 n00 log_or se phi p_fisher [q] status' as
    '%s %s %d %d %d %d %d %d %d %.6f %.6f %.6f %.3E [%.3E] %d' (the positions 1-based; 'nan' as Python spells it where the pair has no
    value; `pairs` of cooccur_reads_llr)"""
    q_cols, q_fmt = T.sci_if(pairs, 'q')
    T.write_rows(path, '%s %s %d %d %d %d %d %d %d %.6f %.6f %.6f %s ' + q_fmt + '%d\n',
                 T.site_cols(pairs, pos=('pos_a', 'pos_b')) + T.fields(pairs, 'dist', 'n11', 'n10', 'n01', 'n00', 'log_or', 'se', 'phi') +
                 [T.sci(pairs['p_fisher'])] + q_cols + T.fields(pairs, 'status'))


def write_site_linkage(path, pairs):
    """<FileID>_site_linkage.txt: per pair 'chrom strand pos_a+1 pos_b+1 dist n_cov pa pb d d_lo d_hi r pi11 pi10 pi01 pi00 stat p_indep
    [q_indep] link_status' as '%s %s %d %d %d %d' + ten '%.6f' + '%.3f %.3E [%.3E] %d' (the positions 1-based; 'nan' as Python spells it
    where the pair has no estimate; `pairs` of cooccur_reads_llr(..., soft=True))"""
    q_cols, q_fmt = T.sci_if(pairs, 'q_indep')
    T.write_rows(path, '%s %s %d %d %d %d' + ' %.6f' * 10 + ' %.3f %s ' + q_fmt + '%d\n',
                 T.site_cols(pairs, pos=('pos_a', 'pos_b')) +
                 T.fields(pairs, 'dist', 'n_cov', 'pa', 'pb', 'd', 'd_lo', 'd_hi', 'r', 'pi11', 'pi10', 'pi01', 'pi00', 'stat') +
                 [T.sci(pairs['p_indep'])] + q_cols + T.fields(pairs, 'link_status'))


def read_domains(hoff, site, state, post, site_pos, delta=None):
    """The runs of consecutive entries in state 1 of every read, from nmod_read_hmm's per-entry tracks: a dict of arrays, one entry per
    run: read, first, last (the positions of its first and last site), n_sites and mean_post.  With nmod_read_viterbi's tracks (state
    its path, delta its margins) also min_delta, the smallest margin inside the run; post may then be None (mean_post NaN)."""
    hoff, state = np.asarray(hoff, np.int64), np.asarray(state)
    n = len(state)
    one = state == 1
    row = np.arange(n)
    read_of = np.searchsorted(hoff, row, 'right') - 1
    begins, ends = row == hoff[read_of], row == hoff[read_of + 1] - 1
    first = np.flatnonzero(one & (begins | ~np.concatenate(([False], one[:-1]))))
    last = np.flatnonzero(one & (ends | ~np.concatenate((one[1:], [False]))))
    post = np.full(n, np.nan) if post is None else np.asarray(post, np.float64)
    sums = np.add.reduceat(np.concatenate((post, [0.0])), np.stack((first, last + 1), 1).ravel())[::2] if len(first) else np.zeros(0)
    pos = np.asarray(site_pos, np.int64)[np.asarray(site, np.int64)]
    count = last - first + 1
    res = dict(read=read_of[first], first=pos[first], last=pos[last], n_sites=count, mean_post=sums / count)
    if delta is not None:
        edges = np.stack((first, last + 1), 1).ravel()
        res['min_delta'] = np.minimum.reduceat(np.concatenate((np.asarray(delta, np.float64), [np.inf])), edges)[::2] if len(first) else np.zeros(0)
    return res


def site_prior(pi_hat, n_valid, mean, prior_reads):
    """The per-site shares the read chain takes as its prior (K23) from K14's estimates: pi_hat shrunk towards `mean` with the weight of
    `prior_reads` reads, (n_valid * pi_hat + prior_reads * mean) / (n_valid + prior_reads), NaN where pi_hat is NaN (the entries take
    their opts->pi there).  Pure numpy.  prior_reads > 0 and mean inside (0, 1): an estimate of exactly 0 or 1 from a few reads never
    becomes a hard 0 or 1.  n_valid: the site's count of scored reads, >= 0."""
    mean, prior_reads = float(mean), float(prior_reads)
    if not 0.0 < mean < 1.0:
        raise ValueError('site_prior: mean must lie inside (0, 1), not %r' % (mean,))
    if not 0.0 < prior_reads < math.inf:
        raise ValueError('site_prior: prior_reads must be positive and finite, not %r' % (prior_reads,))
    pi_hat, n = np.asarray(pi_hat, np.float64), np.asarray(n_valid, np.float64)
    if pi_hat.shape != n.shape:
        raise ValueError('site_prior: pi_hat and n_valid must have one shape')
    if bool(np.any(~(n >= 0.0))) or bool(np.any((pi_hat < 0.0) | (pi_hat > 1.0))):
        raise ValueError('site_prior: n_valid must be >= 0 and pi_hat a share in 0 .. 1 (or NaN)')
    return (n * pi_hat + prior_reads * mean) / (n + prior_reads)


_site_prior_of = site_prior                       # (smooth_reads_llr has an argument of that name)


def smooth_reads_llr(reads, model, alt_model, *, sites='stoich', pi=None, length=200.0, fit_length=None, call_post=0.9, window='kmer',
                     rescale=None, site_alpha=0.05, thr=2.5, prior=0.5, min_positions=1, device=0, log=print, decode='posterior', fit=None,
                     fix_pi=None, site_prior=False, prior_reads=4.0):
    """Per-read two-state HMM smoothing of the window sums at candidate sites (K19, nmod_read_sites_count / nmod_read_hmm): along each
    molecule, where are the modified stretches, and what is the call at a weak site once its neighbours on the same read are taken into
    account?  The optional rescaling (K11), the window sums (K13) and the candidate sites exactly as in cooccur_reads_llr; then, read by
    read, a two-state chain over the candidate sites the read covers, the emission the likelihood ratio K13 computed, the correlation
    decaying as exp(-distance / length), evaluated by forward-backward on the device and on one stream.
    pi: the stationary modified share; None: the mean of K14's estimates over the candidate sites that have one.  length: the
    correlation length in bases.  fit_length: None, or a list of lengths: the chain's log-likelihood summed over the reads
    (math.fsum) is computed for each and the largest is kept (the first of equals); `profile` reports them all.  call_post: the
    posterior from which an entry is called modified (and canonical at 1 - call_post or below).
    Returns a dict: pi, length, profile (a list of (length, log-likelihood) pairs, empty without fit_length);
      reads: index, chrom, strand, n_sites, n_mod, n_can, n_runs, ll, ll_indep, status (L.HMM_NO_SITE);
      entries: hoff (int64[nreads + 1]), site (the index into `sites`), post, state;
      sites: chrom, strand, pos (0-based), n, n_mod, n_can, share = n_mod / (n_mod + n_can) (NaN without a called entry);
      domains: read_domains' runs.  One summary line goes to `log`.
    decode: 'posterior' (the above), 'viterbi' or 'both'.  'viterbi' and 'both' decode every read's most probable path as well (K20,
    nmod_read_viterbi) at the same pi and length, chosen as above, and add the key `viterbi`, a dict laid out like the result itself:
      reads: index, chrom, strand, n_sites, n_mod, n_runs, vit, status, and with 'both' path_logpost = vit - ll, the log of
        P(the path | the read's scores), as the subtraction gives it;
      entries: hoff, site, path, delta;  sites: chrom, strand, pos, n, n_mod, share = n_mod / n (NaN without an entry);
      domains: read_domains' runs of the path with min_delta (mean_post: the posteriors' mean with 'both', NaN with 'viterbi').
    'viterbi' leaves out reads, entries, sites and domains of the posterior decoding.  One more summary line goes to `log`.
    fit: None, or 'mle': pi and length are fitted by maximum likelihood over all reads (K21, nmod_read_hmm_grad through fit_hmm) from
    the pi and length chosen as above, on the device tensors already there, one call per evaluation; fix_pi keeps pi and fits length
    alone.  The decoding uses the fitted values, the result gains the key `fit` (fit_hmm's dict) and one more line goes to `log`.
    Not together with fit_length.
    site_prior: every candidate site gets a share of its own (K23, the _prior entries of K19 - K21): K14's estimate of the site and its
    count of scored reads, shrunk by site_prior() towards `mean` with the weight of prior_reads reads; `mean` is the pi chosen as above
    (or given), which also stands in at a site without an estimate.  prior_reads=4.0 is a default of judgement, not a measurement.  All three entries take the shares; fit_length works unchanged;
    with fit='mle' the shares are held and the length alone is fitted (fix_pi is implied; an explicit fix_pi=False is refused).  The
    result gains `site_prior`: per candidate site chrom, strand, pos (0-based), pi_hat, n_valid and prior; one more line goes to `log`."""
    if decode not in ('posterior', 'viterbi', 'both'):
        raise ValueError("decode must be 'posterior', 'viterbi' or 'both', not %r" % (decode,))
    if fit not in (None, 'mle'):
        raise ValueError("fit must be None or 'mle', not %r" % (fit,))
    if fit is not None and fit_length is not None:
        raise ValueError('fit and fit_length exclude each other: the fit chooses the length itself')
    if fix_pi and fit is None:
        raise ValueError("fix_pi needs fit='mle'")
    if site_prior:
        if fit is not None and fix_pi is not None and not fix_pi:
            raise ValueError("site_prior holds the shares of the sites: fit='mle' fits the length alone, fix_pi=False cannot be asked for")
        fix_pi = True if fit is not None else fix_pi
        _site_prior_of(np.zeros(0), np.zeros(0), 0.5, prior_reads)                            # the refusal, before any device work
    fix_pi = bool(fix_pi)
    setup = _llr_setup(model, alt_model, window, thr, prior, min_positions, rescale)
    site_alpha = engine._check_alpha(site_alpha)
    _sites_by_stoich(sites)
    grid = None if fit_length is None else [float(v) for v in fit_length]
    if grid is not None and not grid:
        raise ValueError('fit_length must name at least one length')
    for v in (grid or [length]):
        engine._hmm_opts(0.5 if pi is None else pi, v, call_post, ())                         # the refusals, before any device work
    sc = _site_scores(reads, setup, sites, site_alpha, rescale, thr, device, want_share='per_site' if site_prior else pi is None)
    det, names, nreads, d_key = sc['det'], sc['names'], sc['nreads'], sc['d_key']
    if pi is None:
        if sc['site_pi'].numel() == 0:
            raise ValueError('pi=None needs a candidate site with an estimate of its modified share (K14); there is none')
        pi = min(max(float(sc['site_pi'].mean().item()), 1e-9), 1.0 - 1e-9)
    shared = (sc['d_cs'], sc['d_start'], sc['d_off'], sc['llr_win'], d_key)
    hoff, nrows = det.read_sites(*shared)
    prior_kw, prior_out = {}, None
    if site_prior:
        import torch
        prior_out = dict(pi_hat=sc['site_pi_at'].cpu().numpy(), n_valid=sc['site_n_valid_at'].cpu().numpy())
        prior_out['prior'] = _site_prior_of(prior_out['pi_hat'], prior_out['n_valid'], pi, prior_reads)
        prior_kw = dict(site_pi=torch.from_numpy(np.ascontiguousarray(prior_out['prior'])).to(d_key.device))
        known = prior_out['prior'][~np.isnan(prior_out['prior'])]
        log('readhmm: per-site prior: %d of %d candidate site(s) with an estimate, shrunk towards %.6g with the weight of %g read(s); shares %.6g .. %.6g'
            % (len(known), len(prior_out['prior']), pi, float(prior_reads), known.min() if len(known) else math.nan,
               known.max() if len(known) else math.nan))
    profile = []
    if grid is not None:
        for v in grid:
            profile.append((v, math.fsum(det.read_hmm(*shared, hoff, nrows, pi=pi, length=v, call_post=call_post, want=('ll',), **prior_kw)['ll'].cpu().tolist())))
        length = max(profile, key=lambda p: p[1])[0]
    fitted = None
    if fit is not None:
        fitted = fit_hmm(lambda p, v: det.read_hmm_grad(*shared, hoff, nrows, pi=p, length=v, want=('sums',), **prior_kw)['sums'].cpu().tolist(), pi, length,
                         fix_pi=fix_pi)
        pi, length = fitted['pi'], fitted['length']
        log('readhmm: maximum-likelihood fit: pi %.6g (%.6g .. %.6g), length %.6g (%.6g .. %.6g), log-likelihood %.6f; %d evaluation(s), %s; %s'
            % (pi, fitted['pi_lo'], fitted['pi_hi'], length, fitted['length_lo'], fitted['length_hi'], fitted['ll'], fitted['n_eval'],
               'converged' if fitted['converged'] else 'not converged', fitted['status']))
    key = d_key.cpu().numpy()
    if prior_out is not None:
        prior_out.update(engine.key_sites(key, names))
    vit = None
    if decode != 'posterior':
        vit = {f: v.cpu().numpy() for f, v in det.read_viterbi(*shared, hoff, nrows, pi=pi, length=length, **prior_kw).items()}
    if decode == 'viterbi':
        out = dict(pi=pi, length=length, profile=profile, **({} if fitted is None else {'fit': fitted}),
                   **({} if prior_out is None else {'site_prior': prior_out}))
        out['viterbi'] = _viterbi_result(vit, hoff.cpu().numpy(), key, names, reads, nreads, None, None, pi, length, log)
        return out
    res = det.read_hmm(*shared, hoff, nrows, pi=pi, length=length, call_post=call_post, **prior_kw)
    res = {f: v.cpu().numpy() for f, v in res.items()}
    called = (res['site_mod'] + res['site_can']).astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        share = np.where(called > 0, res['site_mod'] / called, np.nan)
    out_sites = dict(engine.key_sites(key, names), n=res['site_n'], n_mod=res['site_mod'], n_can=res['site_can'], share=share)
    table = dict(engine.read_head(reads, nreads), **{f: res[f] for f in L.HMM_READ_FIELDS})
    entries = dict(hoff=hoff.cpu().numpy(), site=res['site'], post=res['post'], state=res['state'])
    domains = read_domains(entries['hoff'], entries['site'], entries['state'], entries['post'], out_sites['pos'])
    log('readhmm: %d read(s), %d candidate site(s), %d entr%s; pi %.6g, length %g%s; %d modified and %d canonical at posterior %g, %d domain(s) on %d read(s)'
        % (nreads, len(key), nrows, 'y' if nrows == 1 else 'ies', pi, length, '' if grid is None else ' (the best of %d)' % len(grid),
           int(table['n_mod'].sum()), int(table['n_can'].sum()), float(call_post), len(domains['read']), int((table['n_runs'] > 0).sum())))
    out = dict(pi=pi, length=length, profile=profile, reads=table, entries=entries, sites=out_sites, domains=domains)
    if fitted is not None:
        out['fit'] = fitted
    if prior_out is not None:
        out['site_prior'] = prior_out
    if vit is not None:
        out['viterbi'] = _viterbi_result(vit, entries['hoff'], key, names, reads, nreads, res['ll'], res['post'], pi, length, log)
    return out


HMM_PI_RANGE, HMM_LENGTH_RANGE = (1e-9, 1.0 - 1e-9), (1e-3, 1e9)      # nmod_read_hmm's ranges of pi and length
FIT_MAX_HALVINGS = 20


def _logit(p):
    return math.log(p) - math.log1p(-p)


def _expit(x):
    return 1.0 / (1.0 + math.exp(-x)) if x >= 0.0 else math.exp(x) / (1.0 + math.exp(x))


def fit_hmm(evaluate, pi0, length0, *, fix_pi=False, tol=1e-10, max_iter=50, ci_level=0.95):
    """The maximum-likelihood fit of the read chain's pi and length (K21) by BHHH steps on eta = logit(pi) and lam = ln(length): a pure
    host function.  evaluate(pi, length) returns the eight sums of nmod_read_hmm_grad (L.HMM_GRAD_SUMS) at those parameters: from the
    device (DeviceDetector.read_hmm_grad(..., want=('sums',))) or from any restatement.
    With g = (SUM g_eta, SUM g_lam) and H the 2 x 2 matrix of the summed products (the outer-product estimate of the information), the
    step is H^-1 g and the criterion g . H^-1 g; the fit stops when the criterion is below `tol` (converged) or after `max_iter` steps.
    A step is halved while SUM ll does not increase, at most 20 times; every trial is one evaluation.  The parameters are clamped to
    nmod_read_hmm's ranges.  One parameter alone is fitted when fix_pi is set, when H's lam entry is 0 (no read has two entries), when
    its eta entry is 0, or when H is singular to working precision (then pi alone); `status` says which and why.
    Returns a dict: pi, length, eta, lam, ll (SUM ll at the result); se_eta, se_lam (from H^-1 at the result, NaN for a parameter that
    was not fitted); pi_lo, pi_hi, length_lo, length_hi (Wald intervals at ci_level on the eta and lam scales, mapped back; the value
    itself for a parameter that was not fitted); trace, a list of (pi, length, SUM ll, criterion) per iterate; n_eval; n_reads and
    n_entries (the sums' last two words); converged; status."""
    from statistics import NormalDist
    pi0, length0, tol, ci_level = float(pi0), float(length0), float(tol), float(ci_level)
    if not HMM_PI_RANGE[0] <= pi0 <= HMM_PI_RANGE[1]:
        raise ValueError('pi0 must lie in 1e-9 .. 1 - 1e-9, not %r' % (pi0,))
    if not HMM_LENGTH_RANGE[0] <= length0 <= HMM_LENGTH_RANGE[1]:
        raise ValueError('length0 must lie in 1e-3 .. 1e9 bases, not %r' % (length0,))
    if not tol > 0.0 or int(max_iter) != max_iter or max_iter < 1 or not 0.0 < ci_level < 1.0:
        raise ValueError('fit_hmm: tol must be positive, max_iter a positive integer and ci_level inside (0, 1)')
    clamp = lambda v, r: min(max(v, r[0]), r[1])
    eta_range, lam_range = tuple(_logit(v) for v in HMM_PI_RANGE), tuple(math.log(v) for v in HMM_LENGTH_RANGE)

    def back(v, rng_t, rng, f):
        """the parameter at v on its unbounded scale: the end of its range itself at or beyond that end"""
        return rng[0] if v <= rng_t[0] else (rng[1] if v >= rng_t[1] else clamp(f(v), rng))

    n_eval = 0

    def sums_at(pi, length):
        nonlocal n_eval
        n_eval += 1
        s = [float(v) for v in evaluate(pi, length)]
        if len(s) != len(L.HMM_GRAD_SUMS):
            raise ValueError('fit_hmm: evaluate must return the %d sums of nmod_read_hmm_grad' % len(L.HMM_GRAD_SUMS))
        return s

    def step_of(s):
        """the free parameters, why, the step H^-1 g on them and the inverse's diagonal"""
        g, h00, h01, h11 = (s[1], s[2]), s[3], s[4], s[5]
        free, why = [0, 1], 'pi and length fitted'
        if fix_pi:
            free, why = [1], 'length fitted alone: pi is fixed'
        if 1 in free and not h11 > 0.0:
            free.remove(1)
            why = 'pi fitted alone: no read has two entries, length is not identified' if free else 'nothing fitted: pi is fixed and length is not identified'
        if 0 in free and not h00 > 0.0:
            free.remove(0)
            why = 'length fitted alone: the gradient in pi is 0 for every read' if free else 'nothing fitted: no read has an entry'
        if len(free) == 2 and not h00 * h11 - h01 * h01 > 1e-12 * h00 * h11:
            free, why = [0], 'pi fitted alone: the information matrix is singular to working precision'
        d, var = [0.0, 0.0], [math.nan, math.nan]
        if len(free) == 2:
            det = h00 * h11 - h01 * h01
            d = [(h11 * g[0] - h01 * g[1]) / det, (h00 * g[1] - h01 * g[0]) / det]
            var = [h11 / det, h00 / det]
        elif free:
            i = free[0]
            d[i], var[i] = g[i] / (h00, h11)[i], 1.0 / (h00, h11)[i]
        return free, why, d, var

    pi, length = pi0, length0
    th = [_logit(pi), math.log(length)]
    s = sums_at(pi, length)
    trace, converged = [], False
    for it in range(int(max_iter) + 1):
        free, status, d, var = step_of(s)
        crit = s[1] * d[0] + s[2] * d[1]
        trace.append((pi, length, s[0], crit))
        if not free:
            break
        if crit < tol:
            converged = True
            break
        if it == int(max_iter):
            status += '; stopped after %d steps' % max_iter
            break
        scale, moved = 1.0, False
        for _ in range(FIT_MAX_HALVINGS + 1):
            cand = [clamp(th[0] + scale * d[0], eta_range), clamp(th[1] + scale * d[1], lam_range)]
            # (a parameter that does not move keeps its value, not the round trip through its scale)
            c_pi = pi if cand[0] == th[0] else back(cand[0], eta_range, HMM_PI_RANGE, _expit)
            c_len = length if cand[1] == th[1] else back(cand[1], lam_range, HMM_LENGTH_RANGE, math.exp)
            if (c_pi, c_len) == (pi, length):
                break
            trial = sums_at(c_pi, c_len)
            if trial[0] > s[0]:
                th, pi, length, s, moved = cand, c_pi, c_len, trial, True
                break
            scale *= 0.5
        if not moved:
            status += '; stopped: no step increases the log-likelihood (a bound of the range, or the precision of the sums)'
            break
    z = NormalDist().inv_cdf(0.5 + 0.5 * ci_level)
    se = [math.sqrt(v) if v == v else math.nan for v in var]
    # the ends of a Wald interval mapped back (the value itself for a parameter that was not fitted); exp must not overflow
    ends = lambda i, f, rng, val: (val, val) if se[i] != se[i] else tuple(clamp(f(th[i] + sgn * z * se[i]), rng) for sgn in (-1.0, 1.0))
    (pi_lo, pi_hi) = ends(0, _expit, HMM_PI_RANGE, pi)
    (len_lo, len_hi) = ends(1, lambda x: math.exp(min(x, 700.0)), HMM_LENGTH_RANGE, length)
    return dict(pi=pi, length=length, eta=th[0], lam=th[1], ll=s[0], se_eta=se[0], se_lam=se[1], pi_lo=pi_lo, pi_hi=pi_hi, length_lo=len_lo,
                length_hi=len_hi, trace=trace, n_eval=n_eval, n_reads=int(s[6]), n_entries=int(s[7]), converged=converged, status=status,
                ci_level=ci_level)


def write_hmm_fit(path, fit):
    """<FileID>_hmm_fit.txt: the trace, one line 'iter pi length ll criterion' per iterate as '%d %.9g %.9g %.6f %.3E'; then
    'pi estimate lo hi se_eta' and 'length estimate lo hi se_lam' as '%s %.9g %.9g %.9g %.6g' ('nan' as Python spells it for a parameter
    that was not fitted); then 'evaluations N converged 0|1 level CI' and 'status TEXT' (`fit` of fit_hmm)"""
    with open(path, 'w') as f:
        f.writelines('%d %.9g %.9g %.6f %.3E\n' % ((i,) + tuple(row)) for i, row in enumerate(fit['trace']))
        f.write('pi %.9g %.9g %.9g %.6g\n' % (fit['pi'], fit['pi_lo'], fit['pi_hi'], fit['se_eta']))
        f.write('length %.9g %.9g %.9g %.6g\n' % (fit['length'], fit['length_lo'], fit['length_hi'], fit['se_lam']))
        f.write('evaluations %d converged %d level %g\n' % (fit['n_eval'], int(fit['converged']), fit['ci_level']))
        f.write('status %s\n' % fit['status'])


def _viterbi_result(vit, hoff, key, names, reads, nreads, ll, post, pi, length, log):
    """smooth_reads_llr's `viterbi` entry from nmod_read_viterbi's outputs (ll, post: nmod_read_hmm's, or None)"""
    with np.errstate(invalid='ignore', divide='ignore'):
        share = np.where(vit['site_n'] > 0, vit['site_mod'] / vit['site_n'].astype(np.float64), np.nan)
    sites = dict(engine.key_sites(key, names), n=vit['site_n'], n_mod=vit['site_mod'], share=share)
    table = dict(engine.read_head(reads, nreads), **{f: vit[f] for f in L.VIT_READ_FIELDS})
    if ll is not None:
        table['path_logpost'] = vit['vit'] - ll
    entries = dict(hoff=hoff, site=vit['site'], path=vit['path'], delta=vit['delta'])
    domains = read_domains(hoff, vit['site'], vit['path'], post, sites['pos'], delta=vit['delta'])
    log('readhmm: Viterbi paths at pi %.6g, length %g: %d modified of %d entr%s, %d domain(s) on %d read(s)'
        % (pi, length, int(table['n_mod'].sum()), len(vit['path']), 'y' if len(vit['path']) == 1 else 'ies', len(domains['read']),
           int((table['n_runs'] > 0).sum())))
    return dict(reads=table, entries=entries, sites=sites, domains=domains)


def write_read_hmm(path, res):
    """<FileID>_read_hmm.txt: per read 'index chrom strand n_sites n_mod n_can n_runs ll ll_indep 2(ll-ll_indep)' as
    '%d %s %s %d %d %d %d %.6f %.6f %.6f' (`res` of smooth_reads_llr)"""
    t = res['reads']
    ll, ind = np.asarray(t['ll'], np.float64), np.asarray(t['ll_indep'], np.float64)
    T.write_rows(path, '%d %s %s %d %d %d %d %.6f %.6f %.6f\n',
                 T.read_cols(t) + T.fields(t, 'n_sites', 'n_mod', 'n_can', 'n_runs') + [ll.tolist(), ind.tolist(), (2.0 * (ll - ind)).tolist()])


def write_read_domains(path, res):
    """<FileID>_read_domains.txt: per run of modified entries 'read chrom strand first+1 last+1 n_sites mean_post' as
    '%d %s %s %d %d %d %.6f' (the positions 1-based; `res` of smooth_reads_llr).  With its `viterbi` entry as `res`
    (<FileID>_read_domains_viterbi.txt) a last column min_delta follows, '%.6f' ('nan' as Python spells it for a mean_post without
    posteriors)"""
    d, t = res['domains'], res['reads']
    read = np.asarray(d['read'], np.int64)
    more = ('min_delta',) if 'min_delta' in d else ()
    T.write_rows(path, '%d %s %s %d %d %d %.6f' + ' %.6f' * len(more) + '\n',
                 [read.tolist(), T.strs(np.asarray(t['chrom'])[read]), T.strs(np.asarray(t['strand'])[read]), T.pos1(d['first']), T.pos1(d['last'])] +
                 T.fields(d, 'n_sites', 'mean_post', *more))


def write_site_hmm(path, res):
    """<FileID>_site_hmm.txt: per candidate site 'chrom strand pos+1 n n_mod n_can share' as '%s %s %d %d %d %d %.6f' (the position
    1-based; share 'nan' where no entry is called; `res` of smooth_reads_llr)"""
    s = res['sites']
    T.write_rows(path, '%s %s %d %d %d %d %.6f\n', T.site_cols(s) + T.fields(s, 'n', 'n_mod', 'n_can', 'share'))


def write_read_viterbi(path, res):
    """<FileID>_read_viterbi.txt: per entry 'read site chrom strand pos+1 path delta' as '%d %d %s %s %d %d %.6f' (site: the index into
    the candidate sites; the position 1-based; `res`: the `viterbi` entry of smooth_reads_llr)"""
    e, s = res['entries'], res['sites']
    hoff, site = np.asarray(e['hoff'], np.int64), np.asarray(e['site'], np.int64)
    read = np.searchsorted(hoff, np.arange(len(site)), 'right') - 1
    T.write_rows(path, '%d %d %s %s %d %d %.6f\n',
                 [read.tolist(), site.tolist(), T.strs(np.asarray(s['chrom'])[site]), T.strs(np.asarray(s['strand'])[site]),
                  T.pos1(np.asarray(s['pos'])[site])] + T.fields(e, 'path', 'delta'))


def write_site_prior(path, res):
    """<FileID>_site_prior.txt: per candidate site 'chrom strand pos+1 n_valid pi_hat prior' as '%s %s %d %d %.9g %.9g' (the position
    1-based; 'nan' twice at a site without an estimate; `res`: smooth_reads_llr's result with site_prior)"""
    s = res['site_prior']
    T.write_rows(path, '%s %s %d %d %.9g %.9g\n', T.site_cols(s) + T.fields(s, 'n_valid', 'pi_hat', 'prior'))


def write_site_viterbi(path, res):
    """<FileID>_site_viterbi.txt: per candidate site 'chrom strand pos+1 n n_mod share' as '%s %s %d %d %d %.6f' (the position 1-based;
    share 'nan' where no read has an entry; `res`: the `viterbi` entry of smooth_reads_llr)"""
    s = res['sites']
    T.write_rows(path, '%s %s %d %d %d %.6f\n', T.site_cols(s) + T.fields(s, 'n', 'n_mod', 'share'))


# ---------------------------------------------------------------------------------------------------------------- K22: classes of reads

CLASS_RANGE = (1e-9, 1.0 - 1e-9)                  # nmod_read_classes_step's range of theta and of the weights
CLASS_START_CLAMP = (0.05, 0.95)                  # K14's share is clamped to this before a start is drawn around it


def _check_fit_classes(tol, max_iter):
    tol = float(tol)
    if not tol >= 0.0 or int(max_iter) != max_iter or max_iter < 1:
        raise ValueError('fit_classes: tol must not be negative and max_iter must be a positive integer')
    return tol


def fit_classes(step, theta0, w0, *, tol=1e-9, max_iter=500):
    """The EM loop of the latent-class mixture over the reads (K22): a pure host function over a callable.  step(theta, w) runs one EM
    step at (theta, w) and returns (theta_out, w_out, sums): from the device (DeviceDetector.read_classes_step, whose tensors stay on
    the device: the loop hands them back as they are and reads `sums` alone, a sequence of host floats whose first word is SUM ll at
    (theta, w)) or from any restatement.
    EM never lowers SUM ll; the loop stops when its rise from one step to the next is at most tol * (|ll| + 1) (converged), or after
    max_iter steps.  Returns a dict: theta and w, the parameters SUM ll was last evaluated at; ll; trace, the list of SUM ll per step;
    sums, the last step's; n_iter, the steps run; converged."""
    tol = _check_fit_classes(tol, max_iter)
    theta, w = theta0, w0
    trace, prev, converged, sums = [], None, False, None
    for _ in range(int(max_iter)):
        theta_n, w_n, sums = step(theta, w)
        sums = [float(v) for v in sums]
        ll = sums[0]
        trace.append(ll)
        if prev is not None and ll - prev <= tol * (abs(ll) + 1.0):
            converged = True
            break
        if len(trace) == int(max_iter):
            break
        prev, theta, w = ll, theta_n, w_n
    return dict(theta=theta, w=w, ll=trace[-1], trace=trace, sums=sums, n_iter=len(trace), converged=converged)


def class_starts(pihat, n_classes, n_init, seed=0):
    """The seeded starts of a fit of n_classes classes: a list of n_init arrays theta0 (float64[nsites, n_classes]).  Start i is
    expit(logit(p_j) + z) with p_j K14's share of site j clamped to 0.05 .. 0.95 (0.5 where pihat is NaN) and z ~ N(0, 1) from
    numpy.random.default_rng([seed, n_classes, i]); the weights of every start are equal."""
    if int(n_classes) != n_classes or not 1 <= int(n_classes) <= L.CLASSES_MAX:
        raise ValueError('classes must be integers in 1 .. %d, not %r' % (L.CLASSES_MAX, n_classes))
    if int(n_init) != n_init or n_init < 1:
        raise ValueError('n_init must be a positive integer, not %r' % (n_init,))
    if int(seed) != seed or seed < 0:
        raise ValueError('seed must be a non-negative integer, not %r' % (seed,))
    p = np.asarray(pihat, np.float64)
    p = np.clip(np.where(p == p, p, 0.5), *CLASS_START_CLAMP)
    base = np.log(p) - np.log1p(-p)
    out = []
    for i in range(int(n_init)):
        z = np.random.default_rng([int(seed), int(n_classes), i]).standard_normal((len(p), int(n_classes)))
        out.append(np.clip(1.0 / (1.0 + np.exp(-(base[:, None] + z))), *CLASS_RANGE))
    return out


def class_order(w):
    """the classes by descending weight, ties by index: the permutation new label -> old label"""
    w = np.asarray(w, np.float64)
    return np.lexsort((np.arange(len(w)), -w))


def class_bic(ll, n_classes, n_sites_with_rows, n_reads):
    """BIC = -2 ll + (C - 1 + C * nsites_with_rows) * ln(R1); +inf without a read that has an entry"""
    if n_reads <= 0:
        return math.inf
    return -2.0 * float(ll) + (int(n_classes) - 1 + int(n_classes) * int(n_sites_with_rows)) * math.log(float(n_reads))


def _classes_list(classes):
    counts = [classes] if isinstance(classes, (int, np.integer)) else list(classes)
    if not counts:
        raise ValueError('classes must name at least one number of classes')
    for c in counts:
        if int(c) != c or not 1 <= int(c) <= L.CLASSES_MAX:
            raise ValueError('classes must be integers in 1 .. %d, not %r' % (L.CLASSES_MAX, c))
    return [int(c) for c in counts]


def choose_classes(fits):
    """From the fits of all starts and counts (dicts with C, start, ll, bic): the best start of every count (the largest ll, the first
    of equals), the profile [(C, ll, bic)] over the counts in the order given, and the chosen fit (the smallest BIC, the first of
    equals)"""
    best = {}
    for f in fits:
        if f['C'] not in best or f['ll'] > best[f['C']]['ll']:
            best[f['C']] = f
    profile = [(c, best[c]['ll'], best[c]['bic']) for c in best]
    chosen = None
    for c in best:
        if chosen is None or best[c]['bic'] < chosen['bic']:
            chosen = best[c]
    return best, profile, chosen


def cluster_reads_llr(reads, model, alt_model, *, sites='stoich', classes=2, n_init=4, seed=0, max_iter=500, tol=1e-9, window='kmer',
                      rescale=None, site_alpha=0.05, thr=2.5, prior=0.5, min_positions=1, device=0, log=print):
    """Latent-class clustering of the reads by their modification pattern (K22, nmod_read_class_rows / nmod_read_classes_step): do the
    reads fall into subpopulations with a modified share of their own at every site, and which read belongs to which?  The optional
    rescaling (K11), the window sums (K13) and the candidate sites exactly as in smooth_reads_llr; then a mixture of C classes over
    the reads, sites independent within a class, fitted by EM on the device: one call per step, theta and the weights stay there and
    4 + C sums come back per step (fit_classes).
    classes: the number of classes, or a list of them: each is fitted and the smallest BIC = -2 ll + (C - 1 + C * sites with a row)
    ln(reads with an entry) is kept; 1 is K14's per-site estimate under independence.  n_init, seed: the starts of every count
    (class_starts); the best final ll is kept, the first of equals.  The classes are labelled by descending weight, ties by index.
    Returns a dict: C, w (float64[C]), theta (float64[nsites, C]), ll, bic;
      fit: one entry per start and count: C, start, w (a tuple, relabelled), ll, bic, n_iter, converged, kept (the start kept for its C);
      reads: index, chrom, strand, n_sites, cls (-1 without an entry), gamma (the posterior of cls; float64[nreads, C]: gamma_all), ll,
        status (L.HMM_NO_SITE);
      sites: chrom, strand, pos (0-based), theta and n (float64[nsites, C] each; n: the expected reads of the class at the site);
      profile: [(C, ll, bic)] over the counts.  One summary line per count and one for the choice go to `log`."""
    import torch
    counts = _classes_list(classes)
    for c in counts:
        class_starts(np.zeros(0), c, n_init, seed)                                            # the refusals, before any device work
    _check_fit_classes(tol, max_iter)
    setup = _llr_setup(model, alt_model, window, thr, prior, min_positions, rescale)
    site_alpha = engine._check_alpha(site_alpha)
    _sites_by_stoich(sites)
    sc = _site_scores(reads, setup, sites, site_alpha, rescale, thr, device, want_share='per_site')
    det, names, nreads, d_key = sc['det'], sc['names'], sc['nreads'], sc['d_key']
    shared = (sc['d_cs'], sc['d_start'], sc['d_off'], sc['llr_win'], d_key)
    hoff, nrows = det.read_sites(*shared)
    rows = det.read_class_rows(*shared, hoff, nrows)
    pihat = sc['site_pi_at'].cpu().numpy()
    nsites = len(pihat)
    with_rows = int((np.diff(rows['soff'].cpu().numpy()) > 0).sum())
    dev = torch.device('cuda', device)

    def step(theta, w):
        res = det.read_classes_step(rows, hoff, theta, w, want=('theta_out', 'w_out', 'sums'))
        return res['theta_out'], res['w_out'], res['sums'].cpu().tolist()

    fits = []
    for c in counts:
        for i, theta0 in enumerate(class_starts(pihat, c, n_init, seed)):
            f = fit_classes(step, torch.from_numpy(theta0.reshape(-1)).to(dev), torch.full((c,), 1.0 / c, dtype=torch.float64, device=dev),
                            tol=tol, max_iter=max_iter)
            f.update(C=c, start=i, bic=class_bic(f['ll'], c, with_rows, int(f['sums'][1])))
            fits.append(f)
    best, profile, chosen = choose_classes(fits)
    table_fit = []
    for f in fits:
        order = class_order(f['w'].cpu().numpy())
        table_fit.append(dict(C=f['C'], start=f['start'], w=tuple(f['w'].cpu().numpy()[order].tolist()), ll=f['ll'], bic=f['bic'],
                              n_iter=f['n_iter'], converged=f['converged'], kept=best[f['C']] is f))
    for c, ll, bic in profile:
        log('readclasses: %d class(es): log-likelihood %.6f, BIC %.6f; the best of %d start(s), %d step(s), %s'
            % (c, ll, bic, int(n_init), best[c]['n_iter'], 'converged' if best[c]['converged'] else 'not converged'))
    C_ = chosen['C']
    fin = det.read_classes_step(rows, hoff, chosen['theta'], chosen['w'], want=('gamma', 'll', 'cls', 'status', 'n_site'))
    order = class_order(chosen['w'].cpu().numpy())
    rank = np.empty(C_, np.int64)
    rank[order] = np.arange(C_)
    gamma = fin['gamma'].cpu().numpy().reshape(nreads, C_)[:, order]
    cls = fin['cls'].cpu().numpy()
    cls = np.where(cls >= 0, rank[np.maximum(cls, 0)], -1).astype(np.int32)
    n_sites = np.diff(hoff.cpu().numpy()).astype(np.int32)
    table = dict(engine.read_head(reads, nreads), n_sites=n_sites, cls=cls,
                 gamma=np.where(cls >= 0, gamma[np.arange(nreads), np.maximum(cls, 0)], 0.0) if nreads else np.zeros(0), gamma_all=gamma, ll=fin['ll'].cpu().numpy(), status=fin['status'].cpu().numpy())
    theta = chosen['theta'].cpu().numpy().reshape(nsites, C_)[:, order]
    out_sites = dict(engine.key_sites(d_key.cpu().numpy(), names), theta=theta, n=fin['n_site'].cpu().numpy().reshape(nsites, C_)[:, order])
    w = chosen['w'].cpu().numpy()[order]
    log('readclasses: %d read(s), %d with an entry, %d candidate site(s), %d entr%s; %d class(es) kept%s, weights %s'
        % (nreads, int(chosen['sums'][1]), nsites, nrows, 'y' if nrows == 1 else 'ies', C_,
           '' if len(counts) == 1 else ' by BIC of %s' % ', '.join(str(c) for c in counts), ' '.join('%.4f' % v for v in w)))
    return dict(C=C_, w=w, theta=theta, ll=chosen['ll'], bic=chosen['bic'], fit=table_fit, reads=table, sites=out_sites, profile=profile)


def write_read_classes(path, res):
    """<FileID>_read_classes.txt: a header line, then per read 'read chrom strand n_sites class gamma ll', tab-separated, as
    '%d %s %s %d %d %.6f %.6f' (class -1 and gamma 0 for a read without an entry; `res` of cluster_reads_llr)"""
    t = res['reads']
    T.write_rows(path, '%d\t%s\t%s\t%d\t%d\t%.6f\t%.6f\n', T.read_cols(t) + T.fields(t, 'n_sites', 'cls', 'gamma', 'll'),
                 header='read\tchrom\tstrand\tn_sites\tclass\tgamma\tll\n')


def write_class_sites(path, res):
    """<FileID>_class_sites.txt: a header line, then per candidate site 'chrom strand pos+1 theta_0 N_0 theta_1 N_1 ...', tab-separated,
    theta as '%.6f' and N as '%.3f' (the position 1-based; `res` of cluster_reads_llr)"""
    s = res['sites']
    theta, n = np.asarray(s['theta'], np.float64), np.asarray(s['n'], np.float64)
    nc = theta.shape[1] if theta.ndim == 2 else int(res['C'])
    per = [col.tolist() for c in range(nc) for col in (theta[:, c], n[:, c])] if len(theta) else []
    T.write_rows(path, '%s\t%s\t%d' + '\t%.6f\t%.3f' * nc + '\n', T.site_cols(s) + per,
                 header='chrom\tstrand\tpos' + ''.join('\ttheta_%d\tN_%d' % (c, c) for c in range(nc)) + '\n')


def write_classes_fit(path, res):
    """<FileID>_classes_fit.txt: a header line, then per start and number of classes 'C start weights ll BIC iterations converged kept',
    tab-separated, the weights as '%.6f' joined by commas, ll and BIC as '%.6f', converged and kept as 0 or 1 (`res` of
    cluster_reads_llr)"""
    with open(path, 'w') as f:
        f.write('C\tstart\tweights\tll\tBIC\titerations\tconverged\tkept\n')
        for r in res['fit']:
            f.write('%d\t%d\t%s\t%.6f\t%.6f\t%d\t%d\t%d\n' % (r['C'], r['start'], ','.join('%.6f' % v for v in r['w']), r['ll'], r['bic'], r['n_iter'],
                                                            int(r['converged']), int(r['kept'])))
