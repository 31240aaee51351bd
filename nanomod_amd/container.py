"""Neutral per-group signal container for the `detect` path.

The reference ingests FAST5/HDF5 (myDetect.py:33-127,547-633); h5py is not part of this build, so
the CLI reads one `.npz` per read group holding what ReadAllFast5 accumulates in memory
(`norm_mean[(chrom,strand)][pos] -> samples`, `base[(chrom,strand)][pos]`) as flat arrays:

    chrom  (U)        strand (U1, '+' / '-')    pos (int64, 0-based)    base (U1)
    off    (int64[n+1], CSR row offsets)        sig (float32 | int16 milli-units | float64)
"""
from __future__ import annotations

import os

import numpy as np

FIELDS = ('chrom', 'strand', 'pos', 'base', 'off', 'sig')
# A read-level container holds the reads themselves (what --fast5Reader returns, one read after the other): per read
#     chrom (U)   strand (U1, '+' / '-')   start (int64, 0-based mapped_start)   off (int64[nreads+1], CSR event offsets)
# per event
#     norm_mean (float64 | float32 | int16 milli-units)   base (S1)
# Read order is the order that decides sample order inside a position.  `detect` groups it on the device.
READ_FIELDS = ('chrom', 'strand', 'start', 'off', 'norm_mean', 'base')


def save_group(path, chrom, strand, pos, base, off, sig):
    np.savez_compressed(path, chrom=np.asarray(chrom), strand=np.asarray(strand), pos=np.asarray(pos, dtype=np.int64),
                        base=np.asarray(base), off=np.asarray(off, dtype=np.int64), sig=np.asarray(sig))


def load_group(path):
    z = np.load(path)
    g = {k: z[k] for k in FIELDS}
    n = len(g['pos'])
    if not (len(g['chrom']) == len(g['strand']) == len(g['base']) == n and len(g['off']) == n + 1
            and g['off'][-1] == len(g['sig'])):
        raise ValueError('%s: inconsistent container' % path)
    return g


def milli_or_same(values):
    """int16 milli-units when every value is k/1000.0 with |k| <= 32767 (NanoMod's 3-dp Events), else the values as given"""
    v = np.asarray(values)
    if v.dtype == np.int16 or v.dtype.kind != 'f':
        return v
    k = np.rint(v.astype(np.float64) * 1000.0)
    if np.all(np.abs(k) <= 32767) and np.array_equal(k / 1000.0, v.astype(np.float64)):
        return k.astype(np.int16)
    return v


def save_reads(path, chrom, strand, start, off, norm_mean, base):
    """A read-level container, uncompressed (a multi-GB load is bounded by I/O, not zlib); values go in as int16 milli-units
    when that is exact."""
    np.savez(path, chrom=np.asarray(chrom).astype(str), strand=np.asarray(strand).astype(str), start=np.asarray(start, dtype=np.int64),
             off=np.asarray(off, dtype=np.int64), norm_mean=milli_or_same(norm_mean), base=np.asarray(base).astype('S1'))


def check_reads(r, what='read set'):
    n = len(r['start'])
    off = r['off']
    if not (len(r['chrom']) == len(r['strand']) == n and len(off) == n + 1 and off[0] == 0 and bool(np.all(np.diff(off) >= 0))
            and off[-1] == len(r['norm_mean']) == len(r['base']) and bool(np.all(np.isin(r['strand'], ('+', '-'))))
            and r['norm_mean'].dtype in (np.float64, np.float32, np.int16)):
        raise ValueError('%s: inconsistent read-level container' % what)
    return r


def load_reads(path):
    z = np.load(path)
    r = {k: z[k] for k in READ_FIELDS}
    r['base'] = r['base'].astype('S1')
    return check_reads(r, path)


def is_read_level(path):
    """a read-level container is told from a per-position one by its fields (start + norm_mean instead of pos + sig)"""
    if not (isinstance(path, str) and path.endswith('.npz')) or not os.path.isfile(path):
        return False
    with np.load(path) as z:
        return 'start' in z.files and 'norm_mean' in z.files


def from_moptions_dataset(ds):
    """The reference's in-memory dataset (myDetect.py:569-572) -> container arrays (for tests / migration)."""
    chrom, strand, pos, base, chunks = [], [], [], [], []
    for sk in sorted(ds['norm_mean'].keys()):
        for pk in sorted(ds['norm_mean'][sk].keys()):
            chrom.append(sk[0]); strand.append(sk[1]); pos.append(pk); base.append(ds['base'][sk][pk])
            chunks.append(np.asarray(ds['norm_mean'][sk][pk], dtype=np.float64))
    off = np.zeros(len(pos) + 1, dtype=np.int64)
    if pos:
        off[1:] = np.cumsum([len(c) for c in chunks])
    sig = np.concatenate(chunks) if chunks else np.zeros(0)
    return dict(chrom=np.array(chrom, dtype=str), strand=np.array(strand, dtype=str), pos=np.array(pos, dtype=np.int64),
                base=np.array(base, dtype=str), off=off, sig=sig)


def gather_rows(sig, off, rows):
    """CSR sub-selection: the rows `rows` (in that order) as a new (sig, off)."""
    lens = off[rows + 1] - off[rows]
    new_off = np.zeros(len(rows) + 1, dtype=np.int64)
    new_off[1:] = np.cumsum(lens)
    if len(rows) == 0:
        return sig[:0], new_off
    if int(rows[-1]) - int(rows[0]) + 1 == len(rows) and (len(rows) == 1 or bool(np.all(np.diff(rows) == 1))):
        return sig[off[rows[0]]:off[rows[-1] + 1]], new_off          # consecutive rows: a view, no gather
    idx = np.repeat(off[rows] - new_off[:-1], lens) + np.arange(new_off[-1], dtype=np.int64)
    return sig[idx], new_off
