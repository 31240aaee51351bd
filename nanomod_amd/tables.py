"""The text tables of the read-level pipelines: one writer of rows and the column helpers its callers share.  A writer names its
columns and its format; the documentation of a file's layout stays in that writer's docstring."""
from __future__ import annotations

import numpy as np


def strs(a):
    return np.asarray(a).astype(str).tolist()


def pos1(a):
    """0-based positions as the 1-based ones every text output shows"""
    return (np.asarray(a, dtype=np.int64) + 1).tolist()


def sci(a):
    """'%.3E', or 'nan' as Python spells it"""
    return ['%.3E' % p if p == p else 'nan' for p in np.asarray(a).tolist()]


def fields(table, *names):
    return [np.asarray(table[f]).tolist() for f in names]


def read_cols(table):
    """index chrom strand of a per-read table"""
    return fields(table, 'index') + [strs(table['chrom']), strs(table['strand'])]


def site_cols(sites, pos=('pos',), base=False):
    """chrom strand pos+1 [base] of a per-site table (`pos`: the position fields, each 1-based in the file)"""
    return [strs(sites['chrom']), strs(sites['strand'])] + [pos1(sites[f]) for f in pos] + ([strs(sites['base'])] if base else [])


def sci_if(table, field):
    """an optional '%.3E' column (q, q_indep): its columns, one or none, and its piece of the format"""
    return ([sci(table[field])], '%s ') if field in table else ([], '')


def write_rows(path, fmt, cols, header=None):
    """`header`, then one line `fmt % row` per row of the columns `cols`; a table without rows leaves the header alone, or an empty file"""
    with open(path, 'w') as f:
        if header is not None:
            f.write(header)
        f.writelines(fmt % row for row in zip(*cols))
