"""Per-read shift and scale against a k-mer model (K11; include/nanomod_hip.h: nmod_rescale_reads).

Events are normalised per read by the median / MAD of the raw signal, so a read's level and gain depend on its own base composition
and on the run.  Before the reads of a sample are compared with a k-mer model of another run (kmermodel.model_profile, `detect1
--refProfile`), every read is put on the model's scale: a clipped weighted linear fit x ~ a + b mu of its event levels against the
model levels of their k-mers, then x' = (x - a) / b.

    model = kmermodel.load_kmer_model('control_kmer_model.npz')
    reads2, table = rescale_reads(container.load_reads('sample_reads.npz'), model)
    group = engine.reads_to_group(reads2)                     # a per-position container for profile / detect1 / kmermodel

The fit and the rescaling run in the HIP library; there is no CPU fallback.
"""
from __future__ import annotations

import numpy as np

from . import _lib as L
from . import engine
from . import tables as T

_REASONS = ((L.RESCALE_TOO_FEW, 'too few events'), (L.RESCALE_DEGENERATE, 'degenerate'), (L.RESCALE_OUT_OF_RANGE, 'scale out of range'),
            (L.RESCALE_TOO_LARGE, 'beyond %d events' % L.MAX_DEEP))


def masked_model(model, min_positions=1):
    """k, center, mean, sd of a k-mer model with the entries resting on fewer than min_positions positions masked to NaN (what
    kmermodel.model_profile leaves out)"""
    mean, sd = np.array(model['mean'], dtype=np.float64), np.array(model['sd'], dtype=np.float64)
    thin = np.asarray(model['n_positions']) < int(min_positions)
    mean[thin] = np.nan
    sd[thin] = np.nan
    return dict(k=int(model['k']), center=int(model['center']), mean=mean, sd=sd)


def select_reads(reads, keep):
    """the reads of a read-level set where `keep` holds, as a new read-level set (order kept)"""
    off = np.asarray(reads['off'], dtype=np.int64)
    idx = np.flatnonzero(keep)
    lens = np.diff(off)[idx]
    new_off = np.zeros(len(idx) + 1, dtype=np.int64)
    new_off[1:] = np.cumsum(lens)
    ev = np.repeat(off[idx] - new_off[:-1], lens) + np.arange(new_off[-1], dtype=np.int64)
    out = {f: np.asarray(reads[f])[idx] for f in ('chrom', 'strand', 'start')}
    if 'name' in reads:
        out['name'] = [reads['name'][i] for i in idx]
    out.update(off=new_off, norm_mean=np.asarray(reads['norm_mean'])[ev], base=np.asarray(reads['base'])[ev])
    return out


def rescale_reads(reads, model, *, weighted=True, clip_sigma=3.0, clip_rounds=2, min_events=50, scale_range=(0.5, 2.0), min_positions=1,
                  drop_failed=False, device=0, log=print):
    """Rescale a read-level set (container.READ_FIELDS) to a k-mer model (kmermodel.KMER_MODEL_FIELDS).  Returns (reads', table):
    reads' is the read set with the rescaled events in the dtype they came in (a failed read unchanged, or left out with
    drop_failed), table a dict of one entry per INPUT read: index, chrom, strand, start, events, n_used, shift, scale, status
    (L.RESCALE_* bits).  One summary line goes to `log`."""
    m = masked_model(model, min_positions)
    res = engine.rescale_reads_host(reads['norm_mean'], reads['off'], reads['base'], m, mode='fit_apply', weighted=weighted,
                                    clip_sigma=clip_sigma, clip_rounds=clip_rounds, min_events=min_events, scale_range=scale_range,
                                    device=device)
    st = res['status']
    n = len(st)
    table = dict(engine.read_head(reads, n, np.asarray(reads['off'], dtype=np.int64)), n_used=res['n_used'], shift=res['shift'], scale=res['scale'],
                 status=st)
    out = dict(reads)
    out['norm_mean'] = res['val']
    failed = (st & L.RESCALE_FAILED) != 0
    if drop_failed and failed.any():
        out = select_reads(out, ~failed)
    why = ', '.join('%d %s' % (int(((st & bit) != 0).sum()), what) for bit, what in _REASONS if ((st & bit) != 0).any())
    log('rescale: %d read(s) fitted, %d failed%s, %d clamped%s'
        % (int((~failed).sum()), int(failed.sum()), (' (' + why + ')') if why else '', int(((st & L.RESCALE_CLAMPED) != 0).sum()),
           '; failed reads dropped' if drop_failed and failed.any() else ''))
    return out, table


def write_read_scale(path, reads, table):
    """<FileID>_read_scale.txt: per read 'index chrom strand start events n_used shift scale status' as
    '%d %s %s %d %d %d %.6f %.6f %d'.  chrom / strand / start come from `reads` when it holds the table's reads (nothing was dropped),
    else from the table itself."""
    src = reads if reads is not None and len(reads['start']) == len(table['index']) else table
    T.write_rows(path, '%d %s %s %d %d %d %.6f %.6f %d\n', T.fields(table, 'index') + [T.strs(src['chrom']), T.strs(src['strand'])] +
                 T.fields(src, 'start') + T.fields(table, 'events', 'n_used', 'shift', 'scale', 'status'))
