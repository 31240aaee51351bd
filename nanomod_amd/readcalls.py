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

_RESCALE_KEYS = ('weighted', 'clip_sigma', 'clip_rounds', 'min_events', 'scale_range')


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
    import torch
    m = _rescale.masked_model(model, min_positions)
    k, center = m['k'], m['center']
    if rescale is not None:
        unknown = sorted(set(rescale) - set(_RESCALE_KEYS))
        if unknown:
            raise ValueError('rescale: unknown option(s) %s; known: %s' % (', '.join(unknown), ', '.join(_RESCALE_KEYS)))
    val = np.ascontiguousarray(reads['norm_mean'])
    if val.dtype not in (np.float32, np.int16, np.float64):
        raise ValueError('reads: norm_mean must be float32, int16 (milli-units) or float64')
    off = np.ascontiguousarray(reads['off'], dtype=np.int64)
    nreads = len(off) - 1
    if nreads < 0 or len(reads['start']) != nreads:
        raise ValueError('reads: off needs nreads + 1 entries')
    base = np.ascontiguousarray(np.asarray(reads['base']).astype('S1')).view(np.uint8)
    if len(base) != len(val) or (nreads and (off[0] != 0 or off[-1] != len(val))):
        raise ValueError('reads: norm_mean and base need one entry per event of off')
    engine._join_warm_up(device)
    det = engine.DeviceDetector(device)
    dev = torch.device('cuda', device)
    t = lambda x: torch.from_numpy(x).to(dev)
    d_val, d_off, d_base, d_mean, d_sd = t(val), t(off), t(base), t(m['mean']), t(m['sd'])
    fit = None
    if rescale is not None:
        fit = det.rescale_reads(d_val, d_off, d_base, d_mean, d_sd, k, center, mode='fit_apply', **rescale)
        d_val = fit['val']
    want = L.CALLS_EVENT_FIELDS if events else ('p_win',)
    calls = det.read_calls(d_val, d_off, d_base, d_mean, d_sd, k, center, nb=nb, alpha=alpha, want=want)
    piv = engine.pivot_reads(reads, device, val=calls['p_win'])
    counts = det.site_calls(piv['sig'], off=piv['off'], alpha=alpha)

    table = dict(index=np.arange(nreads, dtype=np.int64), chrom=np.asarray(reads['chrom']).astype(str), strand=np.asarray(reads['strand']).astype(str),
                 start=np.asarray(reads['start'], dtype=np.int64), events=np.diff(off),
                 **{f: calls[f].cpu().numpy() for f in ('n_sites', 'n_called', 'status')})
    if fit is not None:
        table.update(shift=fit['shift'].cpu().numpy(), scale=fit['scale'].cpu().numpy(), rescale_status=fit['status'].cpu().numpy())
    key = piv['key'].cpu().numpy()
    names = np.array(piv['names'], dtype=str)
    row_off = piv['off'].cpu().numpy()
    sites = dict(chrom=names[key >> 41] if len(key) else np.zeros(0, dtype=str), strand=np.where((key >> 40) & 1, '-', '+').astype('U1'),
                 pos=key & ((1 << 40) - 1), base=piv['base'].cpu().numpy().view('S1').astype('U1'), n_reads=np.diff(row_off).astype(np.int32),
                 **{f: counts[f].cpu().numpy() for f in L.SITE_FIELDS})
    log('readcalls: %d read(s), %d of %d event(s) scored, %d called at alpha %g with %d neighbour(s) a side; %d position(s), %d with a call%s'
        % (nreads, int(table['n_sites'].sum()), len(val), int(table['n_called'].sum()), float(alpha), int(nb), len(key),
           int((sites['n_called'] > 0).sum()),
           '' if fit is None else '; %d read(s) not rescaled' % int(((table['rescale_status'] & L.RESCALE_FAILED) != 0).sum())))
    if events:
        return table, sites, {f: calls[f].cpu().numpy() for f in L.CALLS_EVENT_FIELDS}
    return table, sites


def write_read_calls(path, table):
    """<FileID>_read_calls.txt: per read 'index chrom strand start events n_sites n_called status' as '%d %s %s %d %d %d %d %d'"""
    cols = [np.asarray(table['index']).tolist(), np.asarray(table['chrom']).astype(str).tolist(), np.asarray(table['strand']).astype(str).tolist()] + \
           [np.asarray(table[f]).tolist() for f in ('start', 'events', 'n_sites', 'n_called', 'status')]
    with open(path, 'w') as f:
        f.writelines('%d %s %s %d %d %d %d %d\n' % row for row in zip(*cols))


def write_site_calls(path, sites):
    """<FileID>_site_calls.txt: per position 'chrom strand pos+1 base n_reads n_valid n_called frac' as '%s %s %d %s %d %d %d %.6f' (the
    position 1-based like every text output; frac 'nan' where no read has a scored event)"""
    cols = [np.asarray(sites['chrom']).astype(str).tolist(), np.asarray(sites['strand']).astype(str).tolist(),
            (np.asarray(sites['pos'], dtype=np.int64) + 1).tolist(), np.asarray(sites['base']).astype(str).tolist()] + \
           [np.asarray(sites[f]).tolist() for f in ('n_reads', 'n_valid', 'n_called', 'frac')]
    with open(path, 'w') as f:
        f.writelines('%s %s %d %s %d %d %d %.6f\n' % row for row in zip(*cols))
