"""Batches larger than the persistent grids of K8 (nmod_mix_fraction), K9 (nmod_one_sample) and K10 (nmod_kmer_model), batches past one
stride of the classify kernels of K8, K9 and K14 (nmod_site_stoich), and what they must give.

K8, K9 and K14 define a position's outputs by the position alone (the headers of mix_fraction.hip, one_sample.hip and site_stoich.hip
say so, and test_properties_bit_for_bit, test_every_position_alone_gives_the_same_bits and test_a_rows_bits_depend_on_the_row_alone pin
it).  So a batch whose position i is position idx[i] of a small pool must give every repeat the bits of its first copy, and the first
copies are few enough for the numpy restatements (mix_ref, one_ref, stoich_ref) with the gates of the entries' own GPU tests.  K10 pools
over positions: its int16 expectation is computed here, vectorised, in exact integers.  The batches are built without a Python loop over
their positions.  Nothing here calls the library."""
import functools
from fractions import Fraction

import numpy as np

import kmer_ref as KR
import mix_ref as M
import one_ref as O
import stoich_ref as F

# ------------------------------------------------------------------------------------------------------------------------ the grids
# Restated from the launch code as functions of the CU count; the tests size their batches from these and assert that they did.

CLASSIFY_POSITIONS_PER_CU = 16 * 256              # pos_walk.hpp PosListSpace::fill (mix_fraction.hip, one_sample.hip, site_stoich.hip):
                                                  # the classify grid is at most num_cus * 16 blocks of 256 threads, a thread per position
CLASSIFY_BEYOND = 100000                          # positions past the first stride of the classify grid in the classify batches


def classify_stride(cus):
    return CLASSIFY_POSITIONS_PER_CU * cus


def mix_units(cus):
    """mix_fraction.hip mix_launch: cap = num_cus * 8 blocks of kMixThreads = 256 threads for mix_em_kernel<16> (256 / 16 lane groups a
    block) and mix_em_kernel<64> (256 / 64 waves a block), num_cus * 2 workgroups for mix_stream_kernel (pos_walk.hpp launch_groups / launch_blocks)"""
    return (8 * 16 * cus, 8 * 4 * cus, 2 * cus)


def one_units(cus):
    """one_sample.hip one_launch: cap = num_cus * 8 blocks of kOneThreads = 256 threads for one_wave_kernel<16,16> (16 lane groups a
    block), <64,16> and <64,32> (4 waves a block); num_cus * 2 workgroups for one_block_kernel"""
    return (8 * 16 * cus, 8 * 4 * cus, 8 * 4 * cus, 2 * cus)


def stoich_units(cus):
    """site_stoich.hip nmod_site_stoich: cap = num_cus * 8 blocks of 256 threads for st_reg_kernel<16> and <64>, num_cus * 2 workgroups
    for st_block_kernel"""
    return (8 * 16 * cus, 8 * 4 * cus, 2 * cus)


KM_TILE = 64                                      # kmer_model.hip kKmTile: the positions of a wave's tile
KM_LDS_CODES = 4096                               # kmer_model.hip kKmLdsCodes: the table lives in LDS up to here


def km_i16_positions(cus, ncodes):
    """kmer_model.hip km_launch_i16: persistent_grid(ntiles, kKmWaves = 16, num_cus * (LDS_TABLE ? 1 : 2)) blocks of 16 waves, a tile of
    64 positions per wave and turn: the positions one turn of the whole grid takes"""
    return 16 * cus * (1 if ncodes <= KM_LDS_CODES else 2) * KM_TILE


def km_moments_units(cus):
    """kmer_model.hip nmod_kmer_model: mcap = num_cus * 8 blocks of 256 threads for km_moments_kernel, a wave per position"""
    return 8 * 4 * cus


# --------------------------------------------------------------------------------------------------------------- the repeat builder

def tile_rows(val, off, idx):
    """the batch whose row i is row idx[i] of the CSR (val, off): dict(val, off, idx, ev) with val = the pool's val[ev]"""
    off, idx = np.asarray(off, np.int64), np.asarray(idx, np.int64)
    dlens, dstart = np.diff(off), off[:-1]
    assert idx.ndim == 1 and (len(idx) == 0 or (idx.min() >= 0 and idx.max() < len(dlens)))
    lens = dlens[idx]
    boff = np.zeros(len(idx) + 1, np.int64)
    np.cumsum(lens, out=boff[1:])
    ev = np.repeat(dstart[idx] - boff[:-1], lens) + np.arange(int(boff[-1]), dtype=np.int64)
    return dict(val=np.asarray(val)[ev], off=boff, idx=idx, ev=ev)


def first_copies(key):
    """rep[i]: the first index j with key[j] == key[i]"""
    _, first, inv = np.unique(np.asarray(key), return_index=True, return_inverse=True)
    return first[inv.reshape(-1)]


def sample_copies(off, rep):
    """for every sample of a batch whose rows i and rep[i] are copies of each other: the index of the same sample of row rep[i]"""
    off, rep = np.asarray(off, np.int64), np.asarray(rep, np.int64)
    lens = np.diff(off)
    assert np.array_equal(lens, lens[rep])
    return np.repeat(off[rep] - off[:-1], lens) + np.arange(int(off[-1]) - int(off[0]), dtype=np.int64) + off[0]


def _draw_ids(rng, ids, n, weights=None):
    """n of `ids`, each at least once (where n is below their number — a device of very few CUs — n of them, each once)"""
    ids = np.asarray(ids, np.int64)
    assert len(ids) > 0
    if n < len(ids):
        return rng.permutation(ids)[:n]
    p = None if weights is None else np.asarray(weights, np.float64) / np.sum(weights)
    return np.concatenate([ids, rng.choice(ids, n - len(ids), p=p)])


def grid_counts(units):
    """positions per class: more than twice the units, and no multiple of 4 or 16 (a last wave with idle groups, a last block with idle waves)"""
    return tuple(2 * u + 5 for u in units)


def class_index(ids_by_class, counts, seed, weights_by_class=None):
    """idx of a batch with counts[k] pool positions of class k, every pool position of the class at least once, the classes interleaved
    in a seeded order"""
    rng = np.random.default_rng(seed)
    parts = [_draw_ids(rng, ids, n, None if weights_by_class is None else weights_by_class[k]) for k, (ids, n) in enumerate(zip(ids_by_class, counts)) if n]
    return rng.permutation(np.concatenate(parts))


def classify_index(cus, left_ids, ids_by_class, weights_by_class, seed):
    """(idx, left) of a batch of classify_stride(cus) + CLASSIFY_BEYOND positions: about 95 % are drawn from `left_ids` (left[i] is True:
    the positions the entry answers without a persistent kernel, or that the caller gates off), the rest from the classes by weight, and
    every pool position of every class stands at least once on either side of the stride"""
    rng = np.random.default_rng(seed)
    stride = classify_stride(cus)
    n = stride + CLASSIFY_BEYOND
    ids = np.concatenate([np.asarray(i, np.int64) for i in ids_by_class])
    w = np.concatenate([np.asarray(x, np.float64) for x in weights_by_class])
    assert len(ids) == len(w) and len(ids) <= min(stride, CLASSIFY_BEYOND)
    idx = rng.choice(np.asarray(left_ids, np.int64), n)
    left = np.ones(n, bool)
    rest = np.flatnonzero(rng.random(n) >= 0.95)
    idx[rest] = rng.choice(ids, len(rest), p=w / w.sum())
    left[rest] = False
    for at in (rng.choice(stride, len(ids), replace=False), stride + rng.choice(CLASSIFY_BEYOND, len(ids), replace=False)):
        idx[at] = ids
        left[at] = False
    return idx, left


def _csr(rows, dtype):
    off = np.zeros(len(rows) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    val = np.concatenate([np.asarray(r, dtype) for r in rows]) if off[-1] else np.zeros(0, dtype)
    val, off = np.ascontiguousarray(val, dtype), off
    for a in (val, off):
        a.setflags(write=False)
    return val, off


NP_DTYPE = {'i16': np.int16, 'f32': np.float32, 'f64': np.float64}


def _encode(row16, dtype):
    """an int16 milli-unit row in the dtype under test: the same 3-decimal values as int16, float64, or their float32 images"""
    if dtype == 'i16':
        return np.asarray(row16, np.int16)
    return (np.asarray(row16, np.float64) / 1000.0).astype(NP_DTYPE[dtype])


# --------------------------------------------------------------------------------------------------------------------------- K8

MIX_Y_LENGTHS = ((5, 40), (257, 300), (1025, 1100))       # |Y| per class: 16 lanes (up to 256), a wave (up to 1 024), streaming
MIX_R_LENGTHS = (5, 60)
MIX_PER_CLASS = 16
MIX_FRACTIONS = (0.0, 0.05, 0.5, 1.0)                    # positions of one wave stop at different iterations
MIX_MAX_ITER, MIX_TOL = 40, 1e-6
MIX_GATE_MAX = 0.05
MIX_TINY = ((1, 9), (0, 4), (7, 1), (6, 0), (0, 0), (1, 1))   # (|R|, |Y|) of the positions that are degenerate by size
MIX_OUT_FIELDS = M.FIELDS + ('iters', 'status')


def mix_class_of(ny):
    ny = np.asarray(ny)
    return np.where(ny <= M.SMALL, 0, np.where(ny <= M.WAVE, 1, 2))


@functools.lru_cache(maxsize=None)
def mix_pool(dtype, seed=8100):
    """K8's pool: MIX_PER_CLASS positions per class — planted fractions cycling through MIX_FRACTIONS at 3 .. 5 sigma, the class's
    shortest and longest |Y|, one position with a constant reference group and, for the float dtypes, one with a NaN (in Y, or in R
    for the wave class) — and the positions of MIX_TINY, which the classifier answers.  dict(ref=(val, off), mix=(val, off),
    ref_rows, mix_rows, cls (-1: degenerate by size), kind)"""
    rng = np.random.default_rng(seed)
    ref_rows, mix_rows, cls, kind = [], [], [], []
    for k, (lo, hi) in enumerate(MIX_Y_LENGTHS):
        ny = [lo, hi] + rng.integers(lo, hi + 1, MIX_PER_CLASS - 2).tolist()
        for j in range(MIX_PER_CLASS):
            nr = MIX_R_LENGTHS[j] if j < 2 else int(rng.integers(MIX_R_LENGTHS[0], MIX_R_LENGTHS[1] + 1))
            while True:
                r, y, _ = M.planted_rows(rng, nr, ny[j], MIX_FRACTIONS[j % 4], 3.0 + j % 3)
                if len(np.unique(r)) > 1:
                    break
            name = 'planted'
            if j == MIX_PER_CLASS - 2:
                r, name = np.full(nr, r[0], np.int16), 'constant_ref'
            r, y = _encode(r, dtype), _encode(y, dtype)
            if j == MIX_PER_CLASS - 1 and dtype != 'i16':
                (r if k == 1 else y)[3] = np.nan
                name = 'nan'
            ref_rows.append(r); mix_rows.append(y); cls.append(k); kind.append(name)
    for nr, ny in MIX_TINY:
        r, y, _ = M.planted_rows(rng, nr, ny, 0.5, 3.0)
        ref_rows.append(_encode(r, dtype)); mix_rows.append(_encode(y, dtype)); cls.append(-1); kind.append('tiny')
    dt = NP_DTYPE[dtype]
    return dict(ref=_csr(ref_rows, dt), mix=_csr(mix_rows, dt), ref_rows=ref_rows, mix_rows=mix_rows, cls=np.array(cls), kind=tuple(kind))


def mix_tile(pool, idx):
    """the two CSR inputs of the batch whose position i is pool position idx[i]"""
    r, y = tile_rows(*pool['ref'], idx), tile_rows(*pool['mix'], idx)
    return dict(ref=r['val'], roff=r['off'], mix=y['val'], moff=y['off'], idx=r['idx'])


def mix_grid_batch(dtype, cus, seed=8200):
    """counts of grid_counts(mix_units(cus)) per class, interleaved"""
    pool = mix_pool(dtype)
    ids = [np.flatnonzero(pool['cls'] == k) for k in range(3)]
    b = mix_tile(pool, class_index(ids, grid_counts(mix_units(cus)), seed))
    b['cls'] = pool['cls'][b['idx']]
    return b


def mix_classify_batch(dtype, cus, seed=8300):
    """classify_stride(cus) + CLASSIFY_BEYOND positions, about 95 % of them left out: degenerate by size (|Y| or |R| below 2) with the
    gate on, or gated off — by a gate above gate_max or a NaN gate — whatever their size.  The rest are the pool's positions of every
    class, their gates at or below gate_max (some exactly on it).  Adds gate, and `skipped` / `by_size`: what the classifier must answer"""
    pool = mix_pool(dtype)
    cls = pool['cls']
    ids = [np.flatnonzero(cls == k) for k in range(3)]
    tiny = np.flatnonzero(cls < 0)
    left_ids = np.concatenate([tiny, tiny, ids[0]])                                   # two thirds by size, a third ordinary positions gated off
    idx, left = classify_index(cus, left_ids, ids, [np.full(len(ids[0]), 1.0), np.full(len(ids[1]), 0.02), np.full(len(ids[2]), 0.003)], seed)
    rng = np.random.default_rng(seed + 1)
    n = len(idx)
    gate = rng.random(n) * MIX_GATE_MAX
    gate[rng.random(n) < 0.05] = MIX_GATE_MAX                                           # the bound is inclusive
    u = rng.random(n)
    off_gate = np.where(u < 0.5, MIX_GATE_MAX + 1e-9 + rng.random(n), np.nan)          # a gate above the bound, or a NaN
    skipped = left & ((cls[idx] >= 0) | (rng.random(n) < 0.3))
    gate[skipped] = off_gate[skipped]
    b = mix_tile(pool, idx)
    b.update(gate=gate, skipped=skipped, by_size=~skipped & (cls[idx] < 0), cls=np.where(skipped, -1, cls[idx]))
    return b


# --------------------------------------------------------------------------------------------------------------------------- K9

ONE_LIMITS = (256, 1024, 2048)                    # one_sample.hip kOneSmall, kOneWave, kOneWave2
ONE_LENGTHS = {                                   # float32 / int16: per class, row lengths mixed within it
    0: (3, 3, 3, 4, 16, 17, 33, 64, 100, 255, 256, 256),
    1: (257, 300, 333, 400),
    2: (1025, 1060, 1100),
    3: (2049, 2100, 2200, 5000),                  # paddings of 4 096 and 8 192 on one workgroup
}
ONE_LENGTHS_F64 = (2, 3, 17, 64, 65, 128, 129, 257, 300, 300, 3000)    # every float64 position goes to the workgroup form
ONE_OUT_FIELDS = O.FIELDS + ('status',)


def one_class_of(lens, dtype):
    lens = np.asarray(lens)
    if dtype == 'f64':
        return np.full(lens.shape, 3)
    return np.where(lens <= ONE_LIMITS[0], 0, np.where(lens <= ONE_LIMITS[1], 1, np.where(lens <= ONE_LIMITS[2], 2, 3)))


def block_padding(n):
    """one_block_kernel's P: the power of two from 64 up that holds n keys"""
    p = 64
    while p < n:
        p <<= 1
    return p


@functools.lru_cache(maxsize=None)
def one_pool(dtype, seed=9100):
    """K9's pool on one_ref.grid_rows: the lengths of ONE_LENGTHS (float64: ONE_LENGTHS_F64), a one-sample row (T_NAN), for the float
    dtypes a row with a NaN and one with an infinity, and the rows the classifier answers: ref_sd = 0, ref_sd NaN, an empty row, and one
    whose ref_n is 1 (a bad reference only where ref_n is given).  dict(sig=(val, off), rows, mu, sd, nr, lens, kind)"""
    rng = np.random.default_rng(seed)
    if dtype == 'f64':
        sizes = list(ONE_LENGTHS_F64)
        kind = ['plain'] * len(sizes)
        special = [('one_sample', 1), ('nonfinite', 50), ('nonfinite', 3000)]
    else:
        sizes = [n for k in range(4) for n in ONE_LENGTHS[k]]
        kind = ['plain'] * len(sizes)
        special = [('one_sample', 1), ('nonfinite', 50), ('nonfinite', 300), ('nonfinite', 1060), ('nonfinite', 2100)]
    special += [('sd_zero', 40), ('sd_nan', 7), ('empty', 0), ('ref_n_one', 40)]
    sizes += [n for _, n in special]
    kind += [name for name, _ in special]
    rows16, mu, sd, nr = O.grid_rows(rng, sizes)
    rows = [_encode(r, dtype) for r in rows16]
    for i, name in enumerate(kind):
        if name == 'nonfinite' and dtype != 'i16':
            rows[i][len(rows[i]) // 3] = np.nan if sizes[i] != 300 else np.inf
        elif name == 'sd_zero':
            sd[i] = 0.0
        elif name == 'sd_nan':
            sd[i] = np.nan
        elif name == 'ref_n_one':
            nr[i] = 1
    for a in (mu, sd, nr):
        a.setflags(write=False)
    return dict(sig=_csr(rows, NP_DTYPE[dtype]), rows=rows, mu=mu, sd=sd, nr=nr, lens=np.array(sizes), kind=tuple(kind))


def one_pool_class(pool, dtype, with_n):
    """the class of every pool position, -1 for those the classifier answers"""
    kind = np.array(pool['kind'])
    left = np.isin(kind, ('sd_zero', 'sd_nan', 'empty')) | ((kind == 'ref_n_one') & with_n)
    return np.where(left, -1, one_class_of(pool['lens'], dtype))


def _one_weights(lens, dtype):
    """most rows of a class are its short ones (the samples are what costs time); a quarter of the workgroup class has the larger padding"""
    lens = np.asarray(lens)
    if dtype == 'f64':
        return np.where(lens >= 3000, 1.4, 1.0)
    return np.where(lens <= 17, 1.0, np.where(lens <= 256, 0.15, np.where(lens == 5000, 1.7, 1.0)))


def one_tile(pool, idx):
    t = tile_rows(*pool['sig'], idx)
    return dict(sig=t['val'], off=t['off'], idx=t['idx'], mu=pool['mu'][idx], sd=pool['sd'][idx], nr=pool['nr'][idx])


def one_grid_batch(dtype, cus, with_n, seed=9200):
    """grid_counts(one_units(cus)) positions per class (float64: of the workgroup class alone), and each position the classifier answers
    a few times, interleaved"""
    pool = one_pool(dtype)
    cls = one_pool_class(pool, dtype, with_n)
    ids = [np.flatnonzero(cls == k) for k in range(4)] + [np.flatnonzero(cls < 0)]
    counts = grid_counts(one_units(cus))
    counts = tuple(c if len(i) else 0 for c, i in zip(counts, ids)) + (3 * len(ids[4]),)
    weights = [_one_weights(pool['lens'][i], dtype) for i in ids]
    b = one_tile(pool, class_index(ids, counts, seed, weights))
    b['cls'] = cls[b['idx']]
    return b


def one_classify_batch(dtype, cus, with_n, seed=9300):
    """classify_stride(cus) + CLASSIFY_BEYOND positions, about 95 % of them answered by the classifier (an empty row, ref_sd = 0 or NaN),
    the rest the pool's positions of every class"""
    pool = one_pool(dtype)
    cls = one_pool_class(pool, dtype, with_n)
    ids = [np.flatnonzero(cls == k) for k in range(4)]
    ids = [i for i in ids if len(i)]
    scale = {0: 1.0, 1: 0.03, 2: 0.01, 3: 0.004}
    weights = [_one_weights(pool['lens'][i], dtype) * (1.0 if dtype == 'f64' else scale[int(cls[i[0]])]) for i in ids]
    if dtype == 'f64':
        weights = [np.where(pool['lens'][i] >= 3000, 0.01, w) for i, w in zip(ids, weights)]
    idx, left = classify_index(cus, np.flatnonzero(cls < 0), ids, weights, seed)
    b = one_tile(pool, idx)
    b.update(cls=cls[idx], left=left)
    return b


# -------------------------------------------------------------------------------------------------------------------------- K14

STOICH_LENGTHS = (20, F.SMALL + 1, F.WAVE + 1)    # a row of each class, as test_a_batch_larger_than_the_grids has them
STOICH_PER_CLASS = 16
STOICH_MIN_VALID = 3                              # the default: rows of 0 .. 2 scores are TOO_FEW
STOICH_OUT_FIELDS = F.FIELDS + ('n_valid', 'iters', 'status')


@functools.lru_cache(maxsize=None)
def stoich_pool(seed=1410):
    """K14's pool: STOICH_PER_CLASS rows of each of STOICH_LENGTHS, separations and shares rotating, and rows of 0, 1 and 2 scores (one of
    them with a NaN: n_valid counts the valid scores).  dict(score=(val, off), rows, cls (-1: too few scores), lens)"""
    rng = np.random.default_rng(seed)
    rows, cls = [], []
    for k, n in enumerate(STOICH_LENGTHS):
        for j in range(STOICH_PER_CLASS):
            rows.append(F.simulate_row(rng, n, F.SEPARATIONS[j % 4], (0.5, 0.05, 0.9, 0.0)[(j // 4) % 4])); cls.append(k)
    for r in (np.zeros(0), np.array([1.5]), np.array([-0.5]), np.array([2.0, -1.0]), np.array([0.25, 3.0]), np.array([np.nan, 1.0])):
        rows.append(r); cls.append(-1)
    return dict(score=_csr(rows, np.float64), rows=rows, cls=np.array(cls), lens=np.array([len(r) for r in rows]))


def stoich_classify_batch(cus, seed=1411):
    pool = stoich_pool()
    cls = pool['cls']
    ids = [np.flatnonzero(cls == k) for k in range(3)]
    idx, left = classify_index(cus, np.flatnonzero(cls < 0), ids, [np.full(len(ids[0]), 1.0), np.full(len(ids[1]), 0.02), np.full(len(ids[2]), 0.003)], seed)
    t = tile_rows(*pool['score'], idx)
    return dict(score=t['val'], off=t['off'], idx=t['idx'], cls=cls[idx], left=left)


# -------------------------------------------------------------------------------------------------------------------------- K10

KM_LONG_ROWS = (513, 513, 513, 4097, 4097, 4097)  # a tile's run of samples spans many steps of 512 between tiles that span one


def kmer_grid_npos(cus, ncodes):
    """more than two turns of every wave of km_i16_kernel, and a last tile that is not full"""
    return 2 * km_i16_positions(cus, ncodes) + 37


def kmer_float_npos(cus):
    """more than two turns of every wave of km_moments_kernel, and a last block with idle waves"""
    return 2 * km_moments_units(cus) + 5


def kmer_batch(npos, ncodes, seed, stride=0, bounds=False):
    """K10's int16 batch: rows of 1 .. 11 samples (or all of `stride`), and in CSR form about 1 % empty rows and the rows of KM_LONG_ROWS at
    seeded places; about 1 % of the codes -1 and some codes absent; samples on the milli-grid around a level per code, spread 0.2, 1 % of
    them anywhere in +-5, eight at +-32.767, clipped to |k| <= 32 767.  bounds: keep_lo / keep_hi on the 3-decimal grid a quarter unit around the level, so
    that samples stand exactly on them; code 3 has a NaN bound, code 5 none below, code 6 a single kept value.
    dict(sig, off (None with a stride), lens, code, ncodes, stride, keep_lo, keep_hi)"""
    rng = np.random.default_rng(seed)
    if stride:
        lens = np.full(npos, stride, np.int64)
    else:
        lens = rng.integers(1, 12, npos)
        lens[rng.random(npos) < 0.01] = 0
        lens[rng.choice(npos, len(KM_LONG_ROWS), replace=False)] = KM_LONG_ROWS
    code = rng.integers(0, ncodes, npos).astype(np.int32)
    if ncodes >= 64:
        code[code == 7] = 8                                                             # some codes are absent
    code[rng.random(npos) < 0.01] = -1
    off = np.zeros(npos + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    total = int(off[-1])
    level = rng.normal(0.0, 1.0, ncodes)
    row = np.repeat(np.arange(npos), lens)
    k = np.rint(1000.0 * (level[np.maximum(code, 0)][row] + 0.2 * rng.standard_normal(total)))
    out = rng.random(total) < 0.01
    k[out] = np.rint(1000.0 * rng.uniform(-5.0, 5.0, int(out.sum())))
    k[rng.choice(total, 8, replace=False)] = np.tile([32767.0, -32767.0], 4)        # the ends of the range
    sig = np.clip(k, -32767, 32767).astype(np.int16)
    lo = hi = None
    if bounds:
        lo, hi = np.rint(1000.0 * (level - 0.25)) / 1000.0, np.rint(1000.0 * (level + 0.25)) / 1000.0
        if ncodes > 6:
            lo[3] = np.nan
            lo[5] = -np.inf
            hi[6] = lo[6] = np.rint(1000.0 * level[6]) / 1000.0
    return dict(sig=sig, off=None if stride else off, lens=lens, code=code, ncodes=ncodes, stride=stride, keep_lo=lo, keep_hi=hi)


def kmer_expected_i16(sig, lens, code, ncodes, keep_lo=None, keep_hi=None):
    """nmod_kmer_model's definition on int16 rows that follow each other in `sig` from 0 on, vectorised: N, S1, S2, positions and clipped
    per code by np.bincount / np.add.at in int64, then mean and sd per code from Python integers exactly as kmer_ref.kmer_model derives
    them.  |k| <= 32 768, so S2 <= 2^30 per sample: up to 2^33 samples no sum leaves int64 (the batches here stay below 7e6 samples: S2
    below 7.6e15)"""
    sig, lens, code = np.asarray(sig), np.asarray(lens, np.int64), np.asarray(code, np.int64)
    assert sig.dtype == np.int16 and len(sig) == lens.sum() < 2 ** 33
    npos = len(lens)
    status = (np.where((code < 0) | (code >= ncodes), KR.NO_CODE, 0) | np.where(lens == 0, KR.EMPTY, 0)
              | np.where(lens > KR.MAX_DEEP, KR.TOO_LARGE, 0)).astype(np.uint8)
    row = np.repeat(np.arange(npos), lens)
    live = status[row] == 0
    c = np.where(live, code[row], 0)
    k = sig.astype(np.int64)
    kept = live
    if keep_lo is not None:
        d = k / 1000.0                                                                  # the double the definition takes the sample as
        with np.errstate(invalid='ignore'):
            kept = live & (np.asarray(keep_lo, np.float64)[c] <= d) & (d <= np.asarray(keep_hi, np.float64)[c])
    ck, kk = c[kept], k[kept]
    n_s = np.bincount(ck, minlength=ncodes).astype(np.int64)
    n_c = np.bincount(c[live & ~kept], minlength=ncodes).astype(np.int64)
    s1, s2 = np.zeros(ncodes, np.int64), np.zeros(ncodes, np.int64)
    np.add.at(s1, ck, kk)
    np.add.at(s2, ck, kk * kk)
    has_kept = np.bincount(row[kept], minlength=npos) > 0
    n_pos = np.bincount(code[has_kept], minlength=ncodes).astype(np.int64)
    mean, sd = np.full(ncodes, np.nan), np.full(ncodes, np.nan)
    for cc in np.flatnonzero(n_s).tolist():
        n, a, b = int(n_s[cc]), int(s1[cc]), int(s2[cc])
        mean[cc] = float(Fraction(a, n) / 1000)
        sd[cc] = float(KR._sqrt_fraction(n * b - a * a) / n / 1000)
    return dict(n_positions=n_pos, n_samples=n_s, n_clipped=n_c, mean=mean, sd=sd, pos_status=status)


def kmer_float_rows(npos, ncodes, dtype, seed):
    """K10's float batch: kmer_batch's rows as k / 1000.0 in `dtype`, three of them with a NaN or an infinity.  (rows, code)"""
    b = kmer_batch(npos, ncodes, seed)
    val = (b['sig'].astype(np.float64) / 1000.0).astype(dtype)
    rows = np.split(val, b['off'][1:-1])
    some = np.flatnonzero(b['lens'] >= 3)
    for i, v in zip(some[[5, len(some) // 2, -5]].tolist(), (np.nan, np.inf, -np.inf)):
        rows[i][1] = v
    return rows, b['code']
