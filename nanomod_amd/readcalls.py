"""Per-read modification calls against a k-mer model (K12; include/nanomod_hip.h: nmod_read_calls, nmod_site_calls).

`detect1` against a k-mer model answers per position, over all reads.  This module gives the single-molecule answer: every event of
every read is scored against the model level of its k-mer (a two-sided normal tail), the scores of the events of the same read within
`nb` are combined by Fisher's method, and an event whose combined p-value is at most `alpha` is called; per position, the share of the
covering reads that are called there.

    model = kmermodel.load_kmer_model('control_kmer_model.npz')
    table, sites = call_reads(container.load_reads('sample_reads.npz'), model, rescale=dict(min_events=50))
    write_read_calls('run_read_calls.txt', table); write_site_calls('run_site_calls.txt', sites)

The rescaling (K11), the calls, the grouping by position and the counts all run in the HIP library on the device, one after the other
on one stream; there is no CPU fallback.  The p-values are per event and per window and are not adjusted for the number of events.
"""
from __future__ import annotations

import numpy as np

from . import _lib as L
from . import engine
from . import rescale as _rescale
from . import tables as T

_RESCALE_KEYS = ('weighted', 'clip_sigma', 'clip_rounds', 'min_events', 'scale_range')


def _known_options(what, given, keys):
    """refuse a dict of options (or None) that names an option outside `keys`"""
    unknown = sorted(set(given or ()) - set(keys))
    if unknown:
        raise ValueError('%s: unknown option(s) %s; known: %s' % (what, ', '.join(unknown), ', '.join(keys)))


def _checked_reads(reads, which):
    """the arrays of a read-level set (container.READ_FIELDS) that K12 and K13 take, checked: val, off, base"""
    missing = [f for f in ('chrom', 'strand', 'start', 'off', 'norm_mean', 'base') if f not in reads]
    if missing:
        raise ValueError('%s is not a read-level set (no %s): per-position containers have no reads' % (which, ', '.join(missing)))
    val = np.ascontiguousarray(reads['norm_mean'])
    if val.dtype not in (np.float32, np.int16, np.float64):
        raise ValueError('%s: norm_mean must be float32, int16 (milli-units) or float64' % which)
    off = np.ascontiguousarray(reads['off'], dtype=np.int64)
    nreads = len(off) - 1
    if nreads < 0 or len(reads['start']) != nreads:
        raise ValueError('%s: off needs nreads + 1 entries' % which)
    base = np.ascontiguousarray(np.asarray(reads['base']).astype('S1')).view(np.uint8)
    if len(base) != len(val) or (nreads and (off[0] != 0 or off[-1] != len(val))):
        raise ValueError('%s: norm_mean and base need one entry per event of off' % which)
    return val, off, base


def _open_device(device):
    """(det, t): a detector on `device` once its warm-up is through, and the upload of a host array to it"""
    import torch
    engine._join_warm_up(device)
    det = engine.DeviceDetector(device)
    dev = torch.device('cuda', device)
    return det, lambda x: torch.from_numpy(x).to(dev)


def _upload_rescaled(det, t, sample, d_mean, d_sd, k, center, rescale):
    """One checked sample (val, off, base) on the device, put on the model's scale (K11) when `rescale` is a dict of fit options:
    (d_val, d_off, d_base, the fit or None)"""
    d_val, d_off, d_base = (t(x) for x in sample)
    fit = None
    if rescale is not None:
        fit = det.rescale_reads(d_val, d_off, d_base, d_mean, d_sd, k, center, mode='fit_apply', **rescale)
        d_val = fit['val']
    return d_val, d_off, d_base, fit


def _read_table(reads, off, calls, fields, fit):
    """the per-read table of call_reads and call_reads_llr: the head, the entry's per-read `fields` and the rescale fit's"""
    table = dict(engine.read_head(reads, len(off) - 1, off), **{f: calls[f].cpu().numpy() for f in fields})
    if fit is not None:
        table.update(shift=fit['shift'].cpu().numpy(), scale=fit['scale'].cpu().numpy(), rescale_status=fit['status'].cpu().numpy())
    return table


def _pivot_sites(piv, counts, fields):
    """the per-position table of call_reads and call_reads_llr from a pivot and the entry's per-position `fields`"""
    return dict(engine.key_sites(piv['key'].cpu().numpy(), piv['names']), base=piv['base'].cpu().numpy().view('S1').astype('U1'),
                n_reads=np.diff(piv['off'].cpu().numpy()).astype(np.int32), **{f: counts[f].cpu().numpy() for f in fields})


def call_reads(reads, model, *, nb=2, alpha=0.01, min_positions=1, rescale=None, events=False, device=0, log=print):
    """Call the events of a read-level set (container.READ_FIELDS) against a k-mer model (kmermodel.KMER_MODEL_FIELDS).
    rescale: None, or a dict of rescale.rescale_reads' fit options (weighted, clip_sigma, clip_rounds, min_events, scale_range): the
    reads are first put on the model's scale on the device (a read whose fit fails is called as it is, its rescale status in the table).
    Returns (table, sites) — and with `events` a third dict of the per-event tracks z, p, p_win (float64, in the reads' event layout):
    table: one entry per read: index, chrom, strand, start, events, n_sites (scored events), n_called, status (L.CALLS_TOO_LARGE) and,
      when rescaled, shift, scale, rescale_status;
    sites: one entry per covered position in the reference's row order (sorted chromosome, '+' before '-', ascending position): chrom,
      strand, pos, base, n_reads (the events there), n_valid (the scored ones), n_called, frac = n_called / n_valid (NaN without one).
    One summary line goes to `log`."""
    m = _rescale.masked_model(model, min_positions)
    k, center = m['k'], m['center']
    _known_options('rescale', rescale, _RESCALE_KEYS)
    val, off, base = _checked_reads(reads, 'reads')
    nreads = len(off) - 1
    det, t = _open_device(device)
    d_mean, d_sd = t(m['mean']), t(m['sd'])
    d_val, d_off, d_base, fit = _upload_rescaled(det, t, (val, off, base), d_mean, d_sd, k, center, rescale)
    want = L.CALLS_EVENT_FIELDS if events else ('p_win',)
    calls = det.read_calls(d_val, d_off, d_base, d_mean, d_sd, k, center, nb=nb, alpha=alpha, want=want)
    piv = engine.pivot_reads(reads, device, val=calls['p_win'])
    counts = det.site_calls(piv['sig'], off=piv['off'], alpha=alpha)
    table = _read_table(reads, off, calls, ('n_sites', 'n_called', 'status'), fit)
    sites = _pivot_sites(piv, counts, L.SITE_FIELDS)
    log('readcalls: %d read(s), %d of %d event(s) scored, %d called at alpha %g with %d neighbour(s) a side; %d position(s), %d with a call%s'
        % (nreads, int(table['n_sites'].sum()), len(val), int(table['n_called'].sum()), float(alpha), int(nb), len(sites['pos']),
           int((sites['n_called'] > 0).sum()),
           '' if fit is None else '; %d read(s) not rescaled' % int(((table['rescale_status'] & L.RESCALE_FAILED) != 0).sum())))
    if events:
        return table, sites, {f: calls[f].cpu().numpy() for f in L.CALLS_EVENT_FIELDS}
    return table, sites


def write_read_calls(path, table):
    """<FileID>_read_calls.txt: per read 'index chrom strand start events n_sites n_called status' as '%d %s %s %d %d %d %d %d'"""
    T.write_rows(path, '%d %s %s %d %d %d %d %d\n', T.read_cols(table) + T.fields(table, 'start', 'events', 'n_sites', 'n_called', 'status'))


def write_site_calls(path, sites):
    """<FileID>_site_calls.txt: per position 'chrom strand pos+1 base n_reads n_valid n_called frac' as '%s %s %d %s %d %d %d %.6f' (the
    position 1-based like every text output; frac 'nan' where no read has a scored event)"""
    T.write_rows(path, '%s %s %d %s %d %d %d %.6f\n', T.site_cols(sites, base=True) + T.fields(sites, 'n_reads', 'n_valid', 'n_called', 'frac'))
