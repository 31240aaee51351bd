"""The definition nmod_pivot_reads is held to, as vectorised numpy: what fast5_ingest.GroupBuilder builds read by read
(myDetect.py:104-124), without its per-read Python loop and without its per-read filters (fast5_ingest.select_reads applies
those to a read-level set).  Event i of a read of n events starting at s lies at s + i on '+' and s + n - 1 - i on '-'; an
optional inclusive window drops events outside it; rows come ordered by (chrom, strand, pos) with '+' before '-', samples
inside a row in read order, the row's base from its last read.  Nothing of the library is used (test_pivot_ref.py holds it
to GroupBuilder on a machine without a GPU)."""
import numpy as np

FIELDS = ('chrom', 'strand', 'pos', 'base', 'off', 'sig')


def exact_values(v):
    """the float64 values a read set's events stand for: int16 holds milli-units"""
    v = np.asarray(v)
    return v.astype(np.float64) / 1000.0 if v.dtype == np.int16 else v.astype(np.float64)


def pivot_ref(reads, pos_lo=None, pos_hi=None):
    """reads: chrom / strand / start per read, off (nreads + 1), norm_mean and base per event.  Returns the dict of
    GroupBuilder.finish(): chrom, strand, pos, base per row, off, sig (float64)."""
    chrom = np.asarray(reads['chrom']).astype(str)
    minus = np.asarray(reads['strand']).astype(str) == '-'
    start = np.asarray(reads['start'], dtype=np.int64)
    off = np.asarray(reads['off'], dtype=np.int64)
    lens = np.diff(off)
    nev = int(off[-1]) if len(off) else 0
    val = exact_values(reads['norm_mean'])[:nev]
    base = np.asarray(reads['base']).astype('S1').astype('U1')[:nev]
    read = np.repeat(np.arange(len(start)), lens)                       # the read of every event; events are in read order
    i = np.arange(nev, dtype=np.int64) - np.repeat(off[:-1], lens)
    pos = np.where(minus[read], start[read] + lens[read] - 1 - i, start[read] + i)
    keep = np.ones(nev, dtype=bool)
    if pos_lo is not None:
        keep &= pos >= pos_lo
    if pos_hi is not None:
        keep &= pos <= pos_hi
    read, pos, val, base = read[keep], pos[keep], val[keep], base[keep]
    names, cid = np.unique(chrom, return_inverse=True)                  # sorted names: the order of the rows
    order = np.lexsort((pos, minus[read], cid[read]))                   # stable: equal (chrom, strand, pos) stay in read order
    read, pos, val, base = read[order], pos[order], val[order], base[order]
    first = np.ones(len(pos), dtype=bool)
    first[1:] = (cid[read][1:] != cid[read][:-1]) | (minus[read][1:] != minus[read][:-1]) | (pos[1:] != pos[:-1])
    starts = np.flatnonzero(first)
    out_off = np.append(starts, len(pos)).astype(np.int64)
    head = read[starts]
    return dict(chrom=chrom[head], strand=np.where(minus[head], '-', '+').astype('U1'), pos=pos[starts],
                base=base[out_off[1:] - 1], off=out_off, sig=val)


def same_group(got, exp):
    """field for field, float64 samples bit for bit (both sides copy the input values)"""
    for k in FIELDS:
        g, e = np.asarray(got[k]), np.asarray(exp[k])
        assert g.shape == e.shape, (k, g.shape, e.shape)
        assert np.array_equal(g, e), k
    assert np.asarray(got['sig']).dtype == np.float64 and np.asarray(got['off']).dtype == np.int64
    assert np.asarray(got['pos']).dtype == np.int64
