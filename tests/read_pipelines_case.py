"""The eight read-level pipelines on one small input, and their results flattened into a record that can be compared bit for bit
(tests/golden/read_pipelines/; test_read_pipelines_same_gpu.py).

The inputs are the ones the chain tests build: readllr_ref.chain_inputs(n_reads=120, shift_sd=2.0) and, as the control, canonical reads
from the same seed; the replicated comparison splits them into two plus two samples of 60 reads as test_site_diff_rep_gpu._four_samples
does.  The candidate sites of the pipelines that take some are given: the planted base and bases around it on both strands, so the
candidate set cannot depend on a q-value at the edge of a threshold."""
import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'read_pipelines')
HASH_ABOVE = 32768          # an array of more bytes that the recording commit reproduced bit for bit is stored as its SHA-256
SITE_OFFSETS = (-12, -6, -2, -1, 0, 1, 2, 6, 12)


def _take_reads(reads, lo, hi):
    off = np.asarray(reads['off'], np.int64)
    return dict(chrom=reads['chrom'][lo:hi], strand=reads['strand'][lo:hi], start=reads['start'][lo:hi], off=off[lo:hi + 1] - off[lo],
                norm_mean=reads['norm_mean'][off[lo]:off[hi]], base=reads['base'][off[lo]:off[hi]])


def inputs():
    import readllr_ref as RF
    mod, model, alt, planted = RF.chain_inputs(n_reads=120, shift_sd=2.0)
    canon, _, _, planted0 = RF.chain_inputs(n_reads=240, shift_sd=0.0)
    assert planted0 == planted
    pos = np.array([planted + d for d in SITE_OFFSETS] * 2, np.int64)
    sites = (np.array(['chrT'] * len(pos)), np.array(['+'] * len(SITE_OFFSETS) + ['-'] * len(SITE_OFFSETS)), pos)
    return dict(mod=mod, canon=_take_reads(canon, 120, 240), model=model, alt=alt, sites=sites,
                control=[_take_reads(canon, 120, 180), _take_reads(canon, 180, 240)], other=[_take_reads(mod, 0, 60), _take_reads(mod, 60, 120)])


def pipelines(inp):
    """(name, call) of the eight pipelines; call(log) returns the pipeline's result"""
    from nanomod_amd import readcalls as RC
    from nanomod_amd import readllr as RL
    mod, model, alt, sites = inp['mod'], inp['model'], inp['alt'], inp['sites']
    return [
        ('call_reads', lambda log: RC.call_reads(mod, model, rescale={}, log=log)),
        ('call_reads_llr', lambda log: RL.call_reads_llr(mod, model, alt, rescale={}, stoich={}, events=True, log=log)),
        ('compare_reads_llr', lambda log: RL.compare_reads_llr(inp['canon'], mod, model, alt, fdr='bh', min_coverage=5, log=log)),
        ('compare_reads_llr_rep', lambda log: RL.compare_reads_llr_rep(inp['control'], inp['other'], model, alt, fdr='bh', min_coverage=5, log=log)),
        ('cooccur_reads_llr', lambda log: RL.cooccur_reads_llr(mod, model, alt, sites=sites, soft=True, fdr='bh', log=log)),
        ('smooth_both_fit_length', lambda log: RL.smooth_reads_llr(mod, model, alt, sites=sites, decode='both', fit_length=[100.0, 200.0], log=log)),
        ('smooth_site_prior', lambda log: RL.smooth_reads_llr(mod, model, alt, sites=sites, site_prior=True, log=log)),
        ('cluster_reads_llr', lambda log: RL.cluster_reads_llr(mod, model, alt, sites=sites, classes=[1, 2], n_init=2, log=log)),
    ]


def flatten(res, prefix, arrays, keys):
    """every array of a result under its path in `arrays`, the keys of every dict in their order under the dict's path in `keys`"""
    if isinstance(res, dict):
        keys[prefix] = [str(k) for k in res]
        for k, v in res.items():
            flatten(v, '%s/%s' % (prefix, k), arrays, keys)
    elif isinstance(res, (list, tuple)) and res and isinstance(res[0], dict):
        keys[prefix] = len(res)
        for i, v in enumerate(res):
            flatten(v, '%s/%d' % (prefix, i), arrays, keys)
    else:
        a = np.asarray(res)
        assert a.dtype != object, prefix
        arrays[prefix] = a


def run_all(inp=None):
    """-> (arrays, text): arrays the flattened results of all eight pipelines, text a dict of `keys` and the full `log` lines of each"""
    inp = inputs() if inp is None else inp
    arrays, text = {}, {}
    for name, call in pipelines(inp):
        lines, keys = [], {}
        flatten(call(lines.append), name, arrays, keys)
        text[name] = dict(keys=keys, log=lines)
    return arrays, text


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(('%s %s ' % (a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()


def save_record(folder, arrays, text, unstable=()):
    """arrays above HASH_ABOVE bytes (and not in `unstable`) go into the text file as digests, the rest into the .npz"""
    os.makedirs(folder, exist_ok=True)
    hashed = {k: digest(a) for k, a in arrays.items() if a.nbytes > HASH_ABOVE and k not in unstable}
    np.savez_compressed(os.path.join(folder, 'record.npz'), **{k: a for k, a in arrays.items() if k not in hashed})
    with open(os.path.join(folder, 'record.json'), 'w') as f:
        json.dump(dict(pipelines=text, sha256=hashed, unstable=sorted(unstable)), f, indent=1, sort_keys=False)
        f.write('\n')


def load_record(folder=GOLDEN):
    with np.load(os.path.join(folder, 'record.npz')) as z:
        arrays = {k: z[k] for k in z.files}
    with open(os.path.join(folder, 'record.json')) as f:
        return arrays, json.load(f)
