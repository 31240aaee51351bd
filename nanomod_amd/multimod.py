"""Several modifications at once (K26) above the engine: the chain of readllr's multi-table call — one walk over the reads against all
alternative tables (nmod_read_llr_multi), the pivots, the per-state counts and, on request, the shares of all states per site
(nmod_site_compose) — and the writers of its three files (readllr hands them on under its own name)."""
from __future__ import annotations

import math

import numpy as np

from . import _lib as L
from . import engine
from . import tables as T
from .readcalls import _checked_reads, _open_device, _pivot_sites, _read_table, _upload_rescaled

_COMPOSE_KEYS = ('min_valid', 'max_iter', 'tol')
_COMPOSE_DEFAULTS = (3, 500, 1e-9)


def _state_names(names, n_alt):
    names = ['mod%d' % (m + 1) for m in range(n_alt)] if names is None else [str(n) for n in names]
    if len(names) != n_alt or len(set(names)) != n_alt or any(not n.replace('_', '').isalnum() or n == 'can' for n in names):
        raise ValueError("names: one distinct name of letters, digits and '_' per alternative model (and not 'can')")
    return names


def _prior_logits(priors, n_alt):
    """the log prior odds of every state against canonical from the prior probabilities of the states (None: all states and canonical
    alike); canonical takes what the states leave"""
    if priors is None:
        return [0.0] * n_alt
    priors = [float(p) for p in priors]
    rest = 1.0 - sum(priors)
    if len(priors) != n_alt or not all(0.0 < p < 1.0 for p in priors) or not rest > 0.0:
        raise ValueError('priors: one probability inside (0, 1) per alternative model, their sum below 1')
    return [math.log(p / rest) for p in priors]


def call_reads_llr_multi(reads, model, alt_models, *, names=None, priors=None, compose=None, window='kmer', thr=2.5, min_positions=1,
                         rescale=None, events=False, fdr=None, fdr_alpha=0.05, device=0, log=print):
    """Call the events of a read-level set between an unmodified k-mer model and SEVERAL modified ones (1 .. L.MULTI_MAX, one k and
    center): per event the state with the largest window sum when it beats canonical and every other state by `thr`, canonical when
    every state loses by thr, neither otherwise.  names: a name per alternative model (default mod1, mod2, ...); priors: the prior
    probability of each state behind the posterior track (None: uniform over canonical and the states; it does not move the calls);
    window, thr, min_positions, rescale, events, device, log: call_reads_llr's.
    Returns (table, sites) — and with `events` a third dict of the per-event tracks llr, llr_win (float64[n_alt, events]), post
    (float64[n_alt + 1, events]) and call (uint8):
    table: one entry per read: index, chrom, strand, start, events, n_sites, n_can, n_mod_<name> per state, status and, when rescaled,
      shift, scale, rescale_status; `names` lists the states;
    sites: one entry per covered position: chrom, strand, pos, base, n_reads, n_valid (the events with an open state), n_can,
      n_<name> per state (the hard calls) and n_ambiguous.
    compose: None, or a dict of engine.site_compose_host's options (min_valid, max_iter, tol; {} for the defaults): the shares of all
      states per position by maximum likelihood over the window sums of all reads (nmod_site_compose) on the same stream; `sites` gains
      pi_can, pi_<name>, ll, stat, stat_<name>, p_<name> (float64), n_fit, n_partial, iters (int32), open_mask and compose_status
      (uint8, L.COMPOSE_* bits); with fdr ('bh' / 'by') also q_<name>, the q-values of each p_<name> track over all positions.
    One summary line goes to `log`."""
    from . import readllr                                        # (its setup pieces; readllr imports this module)
    alt_models = list(alt_models)
    n_alt = len(alt_models)
    if not 1 <= n_alt <= L.MULTI_MAX:
        raise ValueError('call_reads_llr_multi takes 1 .. %d alternative models, not %d' % (L.MULTI_MAX, n_alt))
    names = _state_names(names, n_alt)
    prior_logit = _prior_logits(priors, n_alt)
    setups = [readllr._llr_setup(model, alt, window, thr, 0.5, min_positions, rescale) for alt in alt_models]   # K13's refusals, per pair
    m0, _, k, center, _, opts = setups[0]
    engine._llr_multi_opts((opts.nb_lo, opts.nb_hi), thr, prior_logit, k, center, [(k, center)] * n_alt, ())
    if compose is not None:
        readllr._known_options('compose', compose, _COMPOSE_KEYS)
        engine._compose_opts(n_alt, *(compose.get(key, default) for key, default in zip(_COMPOSE_KEYS, _COMPOSE_DEFAULTS)))
    elif fdr is not None:
        raise ValueError('fdr needs compose: the q-values are those of its p-value tracks')
    if fdr is not None:
        engine._fdr_method(fdr)
    val, off, base = _checked_reads(reads, 'reads')
    nreads = len(off) - 1
    det, t = _open_device(device)
    torch = det.torch
    d_mean, d_sd = t(m0['mean']), t(m0['sd'])
    d_alt = [(t(s[1]['mean']), t(s[1]['sd'])) for s in setups]
    d_val, d_off, d_base, fit = _upload_rescaled(det, t, (val, off, base), d_mean, d_sd, k, center, rescale)
    want = L.LLR_MULTI_EVENT_FIELDS if events else ('llr_win', 'call')
    calls = det.read_llr_multi(d_val, d_off, d_base, d_mean, d_sd, [a[0] for a in d_alt], [a[1] for a in d_alt], k, center,
                               window=(opts.nb_lo, opts.nb_hi), thr=thr, prior_logit=prior_logit, want=want)

    # the hard calls per position: the call codes pivoted like any event track, then per state an indicator track through nmod_site_llr
    piv = engine.pivot_reads(reads, device, val=calls['call'].to(torch.float64))
    code = piv['sig']
    nan = torch.full_like(code, float('nan'))
    counts = {}
    for m, name in enumerate(['can'] + names):
        ind = torch.where(code == float(m), torch.ones_like(code), torch.where(code == float(L.MULTI_NONE), nan, -torch.ones_like(code)))
        c = det.site_llr(ind, off=piv['off'], thr=0.5)
        counts['n_' + name] = c['n_mod']
        counts['n_valid'] = c['n_valid']
    sites = _pivot_sites(piv, counts, ('n_valid',) + tuple('n_' + n for n in ['can'] + names))
    sites['n_ambiguous'] = (sites['n_valid'] - sum(sites['n_' + n] for n in ['can'] + names)).astype(np.int32)
    sites['names'] = list(names)

    table = _read_table(reads, off, dict(calls, **{'n_mod_' + n: calls['n_mod'][m] for m, n in enumerate(names)}),
                        ('n_sites', 'n_can') + tuple('n_mod_' + n for n in names) + ('status',), fit)
    table['names'] = list(names)
    clause = ''
    if compose is not None:
        rows = [engine.pivot_reads(reads, device, val=calls['llr_win'][m]) for m in range(n_alt)]
        share = det.site_compose([r['sig'] for r in rows], off=piv['off'], **compose)
        sites.update(pi_can=share['pi'][0].cpu().numpy(), ll=share['ll'].cpu().numpy(), stat=share['stat'].cpu().numpy(),
                     n_fit=share['n_valid'].cpu().numpy(), n_partial=share['n_partial'].cpu().numpy(), iters=share['iters'].cpu().numpy(),
                     open_mask=share['open_mask'].cpu().numpy(), compose_status=share['status'].cpu().numpy())
        for m, name in enumerate(names):
            sites.update({'pi_' + name: share['pi'][m + 1].cpu().numpy(), 'stat_' + name: share['stat_m'][m].cpu().numpy(),
                          'p_' + name: share['p_m'][m].cpu().numpy()})
        if fdr is not None:
            tracks = {name: share['p_m'][m].contiguous() for m, name in enumerate(names)}
            qs, _ = det.fdr(tracks, tracks=tuple(names), method=fdr, alpha=fdr_alpha)
            sites.update({'q_' + name: q.cpu().numpy() for name, q in zip(names, qs)})
        clause = '; %d position(s) with shares' % int(((sites['compose_status'] & L.COMPOSE_NO_ESTIMATE) == 0).sum())
    log('readllr: %d read(s), %d of %d event(s) scored against %d modified table(s): %s and %d canonical at threshold %g over %d + 1 + %d '
        'event(s); %d position(s)%s%s'
        % (nreads, int(table['n_sites'].sum()), len(val), n_alt, ', '.join('%d %s' % (int(table['n_mod_' + n].sum()), n) for n in names),
           int(table['n_can'].sum()), float(thr), opts.nb_lo, opts.nb_hi, len(sites['pos']),
           '' if fit is None else '; %d read(s) not rescaled' % int(((table['rescale_status'] & L.RESCALE_FAILED) != 0).sum()), clause))
    if events:
        return table, sites, {f: calls[f].cpu().numpy() for f in L.LLR_MULTI_EVENT_FIELDS}
    return table, sites


def write_read_llr_multi(path, table):
    """<FileID>_read_llr_multi.txt: a header line '#index chrom strand start events n_sites n_can n_mod_<name>... status', then per read
    those columns as '%d %s %s %d %d %d %d' + ' %d' per state + ' %d'"""
    names = list(table['names'])
    cols = ['n_mod_' + n for n in names]
    T.write_rows(path, '%d %s %s %d %d %d %d' + ' %d' * len(names) + ' %d\n',
                 T.read_cols(table) + T.fields(table, 'start', 'events', 'n_sites', 'n_can', *cols, 'status'),
                 header='#index chrom strand start events n_sites n_can ' + ' '.join(cols) + ' status\n')


def write_site_llr_multi(path, sites):
    """<FileID>_site_llr_multi.txt: a header line '#chrom strand pos base n_reads n_valid n_can n_<name>... n_ambiguous', then per position
    those columns (the position 1-based like every text output)"""
    cols = ['n_' + n for n in sites['names']]
    T.write_rows(path, '%s %s %d %s %d %d %d' + ' %d' * len(cols) + ' %d\n',
                 T.site_cols(sites, base=True) + T.fields(sites, 'n_reads', 'n_valid', 'n_can', *cols, 'n_ambiguous'),
                 header='#chrom strand pos base n_reads n_valid n_can ' + ' '.join(cols) + ' n_ambiguous\n')


def write_site_compose(path, sites):
    """<FileID>_site_compose.txt: a header line, then per position 'chrom strand pos+1 base n_reads n_fit n_partial pi_can', per state
    'pi_<name> stat_<name> p_<name> [q_<name>]' as '%.6f %.3f %.3E [%.3E]', then 'll stat iters open_mask status' ('nan' as Python spells
    it where the position has no estimate or the state is closed; `sites` of call_reads_llr_multi(..., compose=...))"""
    names = list(sites['names'])
    head, cols, fmt = [], [], ''
    for n in names:
        q_cols, q_fmt = T.sci_if(sites, 'q_' + n)
        head += ['pi_' + n, 'stat_' + n, 'p_' + n] + (['q_' + n] if q_cols else [])
        cols += T.fields(sites, 'pi_' + n, 'stat_' + n) + [T.sci(sites['p_' + n])] + q_cols
        fmt += '%.6f %.3f %s ' + q_fmt
    T.write_rows(path, '%s %s %d %s %d %d %d %.6f ' + fmt + '%.6f %.3f %d %d %d\n',
                 T.site_cols(sites, base=True) + T.fields(sites, 'n_reads', 'n_fit', 'n_partial', 'pi_can') + cols +
                 T.fields(sites, 'll', 'stat', 'iters', 'open_mask', 'compose_status'),
                 header='#chrom strand pos base n_reads n_fit n_partial pi_can ' + ' '.join(head) + ' ll stat iters open_mask status\n')
