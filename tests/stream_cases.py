"""The stall-and-decoy method behind tests/test_stream_contract_gpu.py: what it takes to see WHERE and WHEN an entry's device work runs.

include/nanomod_hip.h promises of every NMOD_MEM_DEVICE entry that "everything is enqueued on prm->stream, no host read and no
synchronisation".  A test that calls an entry on a side stream whose inputs were settled long before, and then synchronises, cannot
tell: a kernel on the null stream, or a synchronisation inside the entry, gives it the same numbers.  Here the stream is first
occupied by a bounded spin (`stall`), the inputs are put in place BEHIND the spin by copies on that stream (`Swapped.load_real`),
the entry is called, and the inputs are overwritten with another valid batch behind it (`Swapped.load_decoy`):

  * the call returned while the spin was still running (an event recorded behind the spin has not completed): it waited for nothing
    on the stream and read nothing back from it;
  * work the entry put anywhere but on the stream ran during the spin and saw the decoy (or the sentinel the outputs were filled
    with); work that ran later than the call's place in the stream saw the decoy as well.  Either changes a result.

The misses are one-sided: a correct library cannot fail the comparison, and a wrong one fails whenever the spin outlasts the
misplaced work.  The method is blind to work that is misordered but harmless in that schedule: count words zeroed early that are
still zero when they are read, say.  It is also blind to work misplaced on a stream that shares the stalled stream's hardware queue (it is
queued behind the stall after all): the tests run every stalled case on two streams made one after the other.

Call times.  Host-side wall time of one call of each builder below (median of 20, warm, on an MI355X; profiles/stream_contract.txt
has the table and tools/stream_call_times.py measures it):
    fdr_adjust 0.299   mix_fraction 0.032   one_sample 0.037   kmer_model 0.099 (three calls)   rescale_reads 0.034   read_calls 0.033
    site_calls 0.015   read_llr 0.038   site_llr 0.015   site_stoich 0.033   site_diff 0.045   combine_track 0.007   detect_batch 0.154  [ms]
The slowest is 0.299 ms: 50 times that is 15 ms.  T_MS = 100 ms, more than 300 times the slowest call and 50 times the host time of
either pipeline's non-synchronising stages, so that the event check fails falsely only if the host thread is descheduled for a tenth
of a second; with STALL_MARGIN the spin asks for 125 ms, a quarter of STALL_CAP_MS.

Every builder returns (name, make_inputs, call, no_sync):
  make_inputs(part=1)  numpy only: dict(real={name: array}, decoy={name: array}, csr=((offsets name, values name), ...), classes=
                       {label: (class of every row or read, the classes that must occur)}).  part=3: about a third of the batch.
  call(det, t, out=None)  the DeviceDetector method (or the raw C entry) on the tensors t; returns the dict of output tensors; out:
                       such a dict to write into.
  no_sync              the entry promises not to synchronise (every one of these does).
Nothing at import time needs a GPU or torch."""
import ctypes as C
import functools
from collections import namedtuple

import numpy as np

import diff_ref as D
import grid_cases as G
import hist_model as H
import read_batch_cases as RB
import readllr_ref as RL
import stoich_ref as SR
import tail_ref as T

Builder = namedtuple('Builder', 'name make_inputs call no_sync')

STALL_CAP_MS = 500.0                  # the longest stall of one call: a bounded spin, never a hang
STALL_MARGIN = 1.25                   # the spin is asked for this much more than `ms`: "at least ms" under a calibration error
T_MS = 100.0                          # the stall of the contract tests (the docstring says how it was chosen)
SHORT_STALL_MS = 20.0                 # for the entries that synchronise by contract: ordering only
CAL_CYCLES = 1000000                  # the fixed count the calibration times
CAL_SANE_MS = (0.05, 200.0)           # what CAL_CYCLES may take: 0.4 ms at a 2.4 GHz shader clock, 10 ms at a 100 MHz constant clock
CHAIN_OPS = 1 << 24                   # fallback: elements of the float32 buffer of one element-wise op

_cal = {}


def _calibrate(torch, device):
    """ms per unit of spin on `device`, once per session: ('sleep', ms per cycle) or, when torch.cuda._sleep does not keep time,
    ('chain', ms per element-wise op, the buffer).  One synchronisation each."""
    key = str(device)
    if key in _cal:
        return _cal[key]
    with torch.cuda.device(device):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(CAL_CYCLES)                               # (loads the kernel)
        a.record()
        torch.cuda._sleep(CAL_CYCLES)
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        if CAL_SANE_MS[0] <= ms <= CAL_SANE_MS[1]:
            _cal[key] = ('sleep', ms / CAL_CYCLES, None)
        else:
            buf = torch.zeros(CHAIN_OPS, dtype=torch.float32, device=device)
            buf.add_(1.0)
            a.record()
            for _ in range(8):
                buf.add_(1.0)
            b.record()
            b.synchronize()
            per = a.elapsed_time(b) / 8.0
            assert 1e-3 <= per <= 50.0, 'neither torch.cuda._sleep (%g ms) nor an element-wise op (%g ms) keeps time' % (ms, per)
            _cal[key] = ('chain', per, buf)
    return _cal[key]


def stall(stream, ms):
    """occupies `stream` for at least `ms` milliseconds of device time; returns at once on the host"""
    import torch
    assert 0.0 < ms * STALL_MARGIN <= STALL_CAP_MS, 'a stall of %g ms: the cap is %g ms with the margin' % (ms, STALL_CAP_MS)
    kind, per, buf = _calibrate(torch, stream.device)
    with torch.cuda.stream(stream):
        if kind == 'sleep':
            torch.cuda._sleep(int(ms * STALL_MARGIN / per) + 1)
        else:
            for _ in range(int(ms * STALL_MARGIN / per) + 1):
                buf.add_(1.0)


class Swapped:
    """Device input tensors `t` and two contents for them: `real`, the batch under test, and `decoy`, another valid batch of the same
    names, dtypes and lengths.  load_real / load_decoy enqueue device-to-device copies on the current stream."""

    def __init__(self, real, decoy, device='cuda:0'):
        import torch
        assert set(real) == set(decoy)
        up = lambda d: {k: torch.from_numpy(np.array(v, order='C')).to(device) for k, v in d.items()}
        self.real, self.decoy = up(real), up(decoy)
        self.t = {k: torch.empty_like(v) for k, v in self.real.items()}

    def _load(self, src):
        for k, v in src.items():
            self.t[k].copy_(v, non_blocking=True)

    def load_real(self):
        self._load(self.real)

    def load_decoy(self):
        self._load(self.decoy)

    def holds(self, which):
        """whether the inputs hold `which` ('real' / 'decoy') byte for byte; synchronises"""
        import torch
        src = getattr(self, which)
        return all(torch.equal(self.t[k].view(torch.uint8), src[k].view(torch.uint8)) for k in src)


SENTINEL = {'f': -12345.0, 'i': -77, 'u': 0xA5}


def sentinel_value(torch_dtype):
    return SENTINEL['f' if torch_dtype.is_floating_point else 'u' if str(torch_dtype) == 'torch.uint8' else 'i']


def fill_sentinel(out):
    """every tensor of `out` filled with its dtype's sentinel, on the current stream"""
    for v in out.values():
        v.fill_(sentinel_value(v.dtype))
    return out


# ------------------------------------------------------------------------------------------------------------- shared pieces
def reverse_rows(val, off):
    """the CSR (val, off) with its rows in reverse order: the same rows, the same total, other offsets"""
    t = G.tile_rows(val, off, np.arange(len(off) - 1)[::-1])
    return t['val'], t['off']


def _frozen(d):
    for a in d.values():
        a.setflags(write=False)
    return d


def _part(idx, part):
    return idx if part == 1 else idx[:max(len(idx) // part, 1)]


def _tiled_index(n, times, seed):
    return np.random.default_rng(seed).permutation(np.tile(np.arange(n), times))


def _sub(out, prefix):
    """the members of a flat out dict that belong to one sub-call of a builder that makes several"""
    return None if out is None else {k[len(prefix):]: v for k, v in out.items() if k.startswith(prefix)}


def _flat(parts):
    return {p + k: v for p, res in parts.items() for k, v in res.items()}


def stoich_class_of(lens, min_valid=G.STOICH_MIN_VALID):
    lens = np.asarray(lens)
    return np.where(lens < min_valid, -1, np.where(lens <= SR.SMALL, 0, np.where(lens <= SR.WAVE, 1, 2)))


def diff_class_of(n0, n1):
    m = np.maximum(np.asarray(n0), np.asarray(n1))
    return np.where(m <= D.SMALL, 0, np.where(m <= D.WAVE, 1, 2))


def read_class_of(lens):
    return (np.asarray(lens) > RB.WAVE_MAX).astype(np.int64)


RUN_FORMS = ('rank_hist', 'wide', 'rank_pair', 'big')


def run_class_of(n0, n1):
    """the all-tests sorting form of K1 that takes every position (hist_model.instance_of), as an index into RUN_FORMS"""
    return np.array([RUN_FORMS.index(H.instance_of(int(a), int(b))[0]) for a, b in zip(n0, n1)])


# --------------------------------------------------------------------------------------------------------------- det.run
RUN_MAX_N = 2048                      # NMOD_MAX_GROUP: no group beyond it, and the caller says so: none of the three exceptions
RUN_ALPHA = 0.05


@functools.lru_cache(maxsize=None)
def run_inputs(part=1):
    """nmod_detect_batch without its exceptions: float32 CSR rows of 5 .. 300 samples and a few of every larger capacity class up to
    NMOD_MAX_GROUP, every fifth position of group 2 shifted by two units (chain 1 needs positions its q-values reject), four runs"""
    rng = np.random.default_rng(31)
    npos = 300 // part
    n0, n1 = rng.integers(5, 300, npos), rng.integers(5, 300, npos)
    for at, (a, b) in zip(range(3, npos, 17), ((2048, 1500), (400, 512), (700, 1024), (1100, 90), (300, 2048), (1025, 1030)) * 4):
        n0[at], n1[at] = a, b
    off0, off1 = np.zeros(npos + 1, np.int64), np.zeros(npos + 1, np.int64)
    np.cumsum(n0, out=off0[1:]); np.cumsum(n1, out=off1[1:])
    sig0 = np.round(rng.normal(0.0, 1.0, off0[-1]), 3).astype(np.float32)
    shift = np.where(np.arange(npos) % 5 == 0, 2.0, 0.0)
    sig1 = np.round(rng.normal(0.0, 1.0, off1[-1]) + np.repeat(shift, n1), 3).astype(np.float32)
    run = (np.arange(npos) // 80).astype(np.int32)
    real = dict(sig0=sig0, off0=off0, sig1=sig1, off1=off1, run_id=run)
    d0, d1 = reverse_rows(sig0, off0), reverse_rows(sig1, off1)
    decoy = dict(sig0=d0[0], off0=d0[1], sig1=d1[0], off1=d1[1], run_id=(np.arange(npos) // 53).astype(np.int32))
    return dict(real=_frozen(real), decoy=_frozen(decoy), csr=(('off0', 'sig0'), ('off1', 'sig1')),
                classes={'K1 form': (run_class_of(n0, n1), (0, 1, 2))})


def run_call(det, t, out=None):
    return det.run(t['sig0'], t['sig1'], t['run_id'], off0=t['off0'], off1=t['off1'], max_n0=RUN_MAX_N, max_n1=RUN_MAX_N, out=out)


# ------------------------------------------------------------------------------------------------- q-values, window combine
@functools.lru_cache(maxsize=None)
def _k3():
    k3 = T.load_k3()
    names = [T.k3_key(nb, wd, m) + '_in' for nb, wd, m in T.K3_CONFIGS] + ['raw_in', 'conv_in']
    return k3, names


@functools.lru_cache(maxsize=None)
def fdr_inputs(part=1):
    """two tracks of three of tail_ref's K3 input tracks each (more than one tile of the step-up passes), a NaN and a value above 1 every
    few hundred elements; the decoy: the other six tracks"""
    k3, names = _k3()
    cut = lambda p: p[:max(len(p) // part, 1)]
    track = lambda ns: cut(np.concatenate([k3[n] for n in ns]))
    real = dict(p0=track(names[0:3]).copy(), p1=track(names[3:6]).copy())
    decoy = dict(p0=track(names[6:9]).copy(), p1=track(names[9:12]).copy())
    for d in (real, decoy):
        d['p0'][5::301] = np.nan
        d['p1'][7::211] = 1.5
    return dict(real=_frozen(real), decoy=_frozen(decoy), csr=(), classes={})


def fdr_call(det, t, out=None):
    """nmod_fdr_adjust itself, Benjamini-Yekutieli, with the summary"""
    import torch
    from nanomod_amd import _lib as L, engine
    n = t['p0'].numel()
    if out is None:
        out = dict(q0=torch.empty_like(t['p0']), q1=torch.empty_like(t['p1']), summary=torch.empty((2, 4), dtype=torch.float64, device=t['p0'].device))
    parr = (C.c_void_p * 2)(t['p0'].data_ptr(), t['p1'].data_ptr())
    qarr = (C.c_void_p * 2)(out['q0'].data_ptr(), out['q1'].data_ptr())
    engine._call(det.lib, 'nmod_fdr_adjust', det._params(L.DTYPE_F64, 0, 0, 0, 0), n, 2, parr, L.FDR_BY, RUN_ALPHA, qarr, out['summary'].data_ptr())
    return out


@functools.lru_cache(maxsize=None)
def combine_inputs(part=1):
    """tail_ref's K3 inputs: the track with a NaN, a 0 and a 1 next to run breaks under K3's run ids; the decoy: the log-uniform track
    under other breaks"""
    k3, _ = _k3()
    n = T.K3_N // part
    rng = np.random.default_rng(12)
    real = dict(ks_d=rng.random(n), ks_p=k3['conv_in'][:n].copy(), run_id=T.k3_run_id()[:n].copy())
    decoy = dict(ks_d=rng.random(n), ks_p=k3['raw_in'][:n].copy(), run_id=T.k3_run_id(breaks=(100, 512, 900))[:n].copy())
    return dict(real=_frozen(real), decoy=_frozen(decoy), csr=(), classes={})


def combine_call(det, t, out=None):
    """nmod_combine_track itself under the detector's nb / method / weights_dif"""
    import torch
    from nanomod_amd import _lib as L, engine
    if out is None:
        out = dict(comb_st=torch.empty_like(t['ks_p']), comb_p=torch.empty_like(t['ks_p']))
    engine._call(det.lib, 'nmod_combine_track', det._params(L.DTYPE_F64, 0, 0, 0, 0), t['ks_p'].numel(), t['ks_d'].data_ptr(), t['ks_p'].data_ptr(),
                 t['run_id'].data_ptr(), out['comb_st'].data_ptr(), out['comb_p'].data_ptr())
    return out


# --------------------------------------------------------------------------------------------------------------- K8, K9
@functools.lru_cache(maxsize=None)
def mix_inputs(part=1):
    """grid_cases.mix_pool four times over in a seeded order: every class of K8 and the positions its classifier answers; a gate that
    leaves some out.  The decoy: the same positions in reverse order under another gate"""
    pool = G.mix_pool('f32')
    idx = _part(_tiled_index(len(pool['cls']), 4, 81), part)
    rng = np.random.default_rng(82)

    def one(ix):
        b = G.mix_tile(pool, ix)
        gate = rng.random(len(ix)) * 0.07
        gate[rng.random(len(ix)) < 0.1] = np.nan
        return dict(ref=b['ref'], roff=b['roff'], mix=b['mix'], moff=b['moff'], gate=gate)
    real, decoy = one(idx), one(idx[::-1])
    ny = np.diff(real['moff'])
    cls = np.where(pool['cls'][idx] < 0, -1, G.mix_class_of(ny))
    return dict(real=_frozen(real), decoy=_frozen(decoy), csr=(('roff', 'ref'), ('moff', 'mix')), classes={'K8': (cls, (-1, 0, 1, 2))})


def mix_call(det, t, out=None):
    return det.mix(t['ref'], t['mix'], off0=t['roff'], off1=t['moff'], gate=t['gate'], gate_max=G.MIX_GATE_MAX, max_iter=G.MIX_MAX_ITER,
                   tol=G.MIX_TOL, want_resp=True, out=out)


@functools.lru_cache(maxsize=None)
def one_inputs(part=1):
    """grid_cases.one_pool three times over: the four classes of K9 and the positions its classifier answers, a stored control (ref_n)
    and run ids for the combined track"""
    pool = G.one_pool('f32')
    idx = _part(_tiled_index(len(pool['lens']), 3, 91), part)

    def one(ix, run_len):
        b = G.one_tile(pool, ix)
        return dict(sig=b['sig'], off=b['off'], mu=b['mu'].copy(), sd=b['sd'].copy(), nr=b['nr'].astype(np.int32), run_id=(np.arange(len(ix)) // run_len).astype(np.int32))
    real, decoy = one(idx, 37), one(idx[::-1], 23)
    return dict(real=_frozen(real), decoy=_frozen(decoy), csr=(('off', 'sig'),),
                classes={'K9': (G.one_pool_class(pool, 'f32', True)[idx], (-1, 0, 1, 2, 3))})


def one_call(det, t, out=None):
    return det.one_sample(t['sig'], t['mu'], t['sd'], t['nr'], t['run_id'], off=t['off'], out=out)


# ------------------------------------------------------------------------------------------------------------------- K10
KMER_FORMS = (('lds.', 64, True), ('glb.', 8192, False))          # int16: the table in LDS (with bounds), the table in global memory
KMER_NPOS = 600


@functools.lru_cache(maxsize=None)
def kmer_inputs(part=1):
    """three calls of K10: int16 rows with the table in LDS (64 codes, with keep bounds) and in global memory (8 192 codes), and float32
    rows (the moments and combine kernels).  The decoy: the rows in reverse order under the same codes, the bounds moved"""
    real, decoy, csr = {}, {}, []
    classes = {'K10 table': (np.array([int(ncodes > G.KM_LDS_CODES) for _, ncodes, _ in KMER_FORMS]), (0, 1))}
    npos = KMER_NPOS // part
    for prefix, ncodes, bounds in KMER_FORMS:
        b = G.kmer_batch(npos, ncodes, 1000 + ncodes, bounds=bounds)
        rv, ro = reverse_rows(b['sig'], b['off'])
        real.update({prefix + 'sig': b['sig'], prefix + 'off': b['off'], prefix + 'code': b['code']})
        decoy.update({prefix + 'sig': rv, prefix + 'off': ro, prefix + 'code': b['code'].copy()})
        if bounds:
            real.update({prefix + 'lo': b['keep_lo'], prefix + 'hi': b['keep_hi']})
            decoy.update({prefix + 'lo': b['keep_lo'] + 0.05, prefix + 'hi': b['keep_hi'] + 0.05})
        csr.append((prefix + 'off', prefix + 'sig'))
    rows, code = G.kmer_float_rows(npos // 2, 64, np.float32, 1064)
    sig = np.concatenate(rows)
    off = np.zeros(len(rows) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    rv, ro = reverse_rows(sig, off)
    real.update({'f32.sig': sig, 'f32.off': off, 'f32.code': code})
    decoy.update({'f32.sig': rv, 'f32.off': ro, 'f32.code': code.copy()})
    csr.append(('f32.off', 'f32.sig'))
    return dict(real=_frozen(real), decoy=_frozen(decoy), csr=tuple(csr), classes=classes)


def kmer_call(det, t, out=None):
    parts = {}
    for prefix, ncodes, bounds in KMER_FORMS:
        parts[prefix] = det.kmer_model(t[prefix + 'sig'], t[prefix + 'code'], ncodes, t.get(prefix + 'lo'), t.get(prefix + 'hi'), off=t[prefix + 'off'],
                                       out=_sub(out, prefix))
    parts['f32.'] = det.kmer_model(t['f32.sig'], t['f32.code'], 64, off=t['f32.off'], out=_sub(out, 'f32.'))
    return out if out is not None else _flat(parts)


# ------------------------------------------------------------------------------------------------------------ K11, K12, K13
READ_K, READ_CENTER, READ_NB = 3, 1, 2


def _read_inputs(d, idx, tables):
    """the batch of distinct reads d[idx] and, as its decoy, d[idx reversed] against tables moved a little"""
    def one(ix, moved):
        b = RB.tile_batch(d['val'], d['off'], d['base'], ix)
        res = dict(val=b['val'], off=b['off'], base=b['base'])
        for name in tables:
            res[name] = d[name] + 0.05 if moved and 'mean' in name else d[name] * 1.1 if moved else d[name].copy()
        return res
    real, decoy = one(idx, False), one(idx[::-1], True)
    return dict(real=_frozen(real), decoy=_frozen(decoy), csr=(('off', 'val'),),
                classes={'reads': (read_class_of(np.diff(real['off'])), (0, 1))})


@functools.lru_cache(maxsize=None)
def rescale_inputs(part=1):
    """read_batch_cases.rescale_distinct twice over: reads a wave computes and reads a workgroup computes, the failing statuses among them"""
    d = RB.rescale_distinct(READ_K, READ_CENTER, 'float32')
    return _read_inputs(d, _part(_tiled_index(len(d['off']) - 1, 2, 111), part), ('mean', 'sd'))


def rescale_call(det, t, out=None):
    return det.rescale_reads(t['val'], t['off'], t['base'], t['mean'], t['sd'], READ_K, READ_CENTER, min_events=RB.RESCALE_MIN_EVENTS, out=out)


@functools.lru_cache(maxsize=None)
def calls_inputs(part=1):
    """read_batch_cases.calls_distinct twice over: both read classes of K12"""
    d = RB.calls_distinct(READ_K, READ_CENTER, READ_NB, 'float32')
    return _read_inputs(d, _part(_tiled_index(len(d['off']) - 1, 2, 121), part), ('mean', 'sd'))


def calls_call(det, t, out=None):
    return det.read_calls(t['val'], t['off'], t['base'], t['mean'], t['sd'], READ_K, READ_CENTER, nb=READ_NB, alpha=RB.CALLS_ALPHA, out=out)


@functools.lru_cache(maxsize=None)
def llr_inputs(part=1):
    """readllr_ref.parity_inputs: every length at which K13 takes another path, both read classes (part 3: without the two longest reads)"""
    d = RL.parity_inputs(READ_K, READ_CENTER, 'kmer', 'float32')
    n = len(d['off']) - 1
    return _read_inputs(d, np.arange(n if part == 1 else n - 2), ('mean', 'sd', 'alt_mean', 'alt_sd'))


def llr_call(det, t, out=None):
    return det.read_llr(t['val'], t['off'], t['base'], t['mean'], t['sd'], t['alt_mean'], t['alt_sd'], READ_K, READ_CENTER, window='kmer',
                        thr=RL.PARITY_THR, prior_logit=RL.PARITY_PRIOR_LOGIT, out=out)


# ------------------------------------------------------------------------------------------- the per-site entries (K12 .. K15)
def _score_inputs(values_of, part, seed):
    """grid_cases.stoich_pool's rows twice over (every class of K14, and rows of 0 .. 2 scores) holding values_of(pool scores, rng)"""
    pool = G.stoich_pool()
    idx = _part(_tiled_index(len(pool['lens']), 2, seed), part)
    rng = np.random.default_rng(seed + 1)

    def one(ix):
        b = G.tile_rows(*pool['score'], ix)
        return dict(score=values_of(b['val'], rng), off=b['off'])
    real, decoy = one(idx), one(idx[::-1])
    return dict(real=_frozen(real), decoy=_frozen(decoy), csr=(('off', 'score'),), classes={'K14': (stoich_class_of(np.diff(real['off'])), (-1, 0, 1, 2))})


def _as_p(s, rng):
    p = rng.random(len(s)) * np.where(rng.random(len(s)) < 0.3, 0.02, 1.0)
    p[np.isnan(s)] = np.nan
    p[::97] = np.nan
    return p


@functools.lru_cache(maxsize=None)
def site_calls_inputs(part=1):
    return _score_inputs(_as_p, part, 131)


def site_calls_call(det, t, out=None):
    return det.site_calls(t['score'], off=t['off'], alpha=RUN_ALPHA, out=out)


@functools.lru_cache(maxsize=None)
def site_llr_inputs(part=1):
    return _score_inputs(lambda s, rng: s.copy(), part, 141)


def site_llr_call(det, t, out=None):
    return det.site_llr(t['score'], off=t['off'], thr=RL.PARITY_THR, out=out)


@functools.lru_cache(maxsize=None)
def stoich_inputs(part=1):
    return _score_inputs(lambda s, rng: s.copy(), part, 151)


def stoich_call(det, t, out=None):
    return det.site_stoich(t['score'], off=t['off'], resp=True, out=out)


@functools.lru_cache(maxsize=None)
def diff_inputs(part=1):
    """diff_ref.length_batch four times over: every class of K15 by the longer row, lopsided pairs, the LDS stage limit; with the interval"""
    s0, o0, s1, o1 = D.length_batch()
    idx = _part(_tiled_index(len(o0) - 1, 4, 161), part)

    def one(ix):
        a, b = G.tile_rows(s0, o0, ix), G.tile_rows(s1, o1, ix)
        return dict(score0=a['val'], off0=a['off'], score1=b['val'], off1=b['off'])
    real, decoy = one(idx), one(idx[::-1])
    return dict(real=_frozen(real), decoy=_frozen(decoy), csr=(('off0', 'score0'), ('off1', 'score1')),
                classes={'K15': (diff_class_of(np.diff(real['off0']), np.diff(real['off1'])), (0, 1, 2))})


def diff_call(det, t, out=None):
    return det.site_diff(t['score0'], t['score1'], off0=t['off0'], off1=t['off1'], out=out)


# the twelve secondary entries the header promises the stream contract for, and nmod_detect_batch outside its three exceptions
ENTRY_BUILDERS = (
    Builder('fdr_adjust', fdr_inputs, fdr_call, True),
    Builder('mix_fraction', mix_inputs, mix_call, True),
    Builder('one_sample', one_inputs, one_call, True),
    Builder('kmer_model', kmer_inputs, kmer_call, True),
    Builder('rescale_reads', rescale_inputs, rescale_call, True),
    Builder('read_calls', calls_inputs, calls_call, True),
    Builder('site_calls', site_calls_inputs, site_calls_call, True),
    Builder('read_llr', llr_inputs, llr_call, True),
    Builder('site_llr', site_llr_inputs, site_llr_call, True),
    Builder('site_stoich', stoich_inputs, stoich_call, True),
    Builder('site_diff', diff_inputs, diff_call, True),
    Builder('combine_track', combine_inputs, combine_call, True),
)
RUN_BUILDER = Builder('detect_batch', run_inputs, run_call, True)
BUILDERS = ENTRY_BUILDERS + (RUN_BUILDER,)
BY_NAME = {b.name: b for b in BUILDERS}
KERNEL_ENTRIES = ('mix_fraction', 'one_sample', 'kmer_model', 'rescale_reads', 'read_calls', 'site_calls', 'read_llr', 'site_llr', 'site_stoich',
                  'site_diff')                                  # K8 .. K15


# ----------------------------------------------------------------------------------------------------------- the pipelines
CHAIN_MIN_COVERAGE = 5


def _take_reads(reads, lo, hi):
    off = np.asarray(reads['off'], np.int64)
    return dict(chrom=reads['chrom'][lo:hi], strand=reads['strand'][lo:hi], start=reads['start'][lo:hi], off=off[lo:hi + 1] - off[lo],
                norm_mean=reads['norm_mean'][off[lo]:off[hi]], base=reads['base'][off[lo]:off[hi]])


@functools.lru_cache(maxsize=None)
def chain2_inputs():
    """Two samples of 40 int16 reads over one short reference (readllr_ref.chain_inputs): sample 1 half modified at the planted base,
    sample 0 canonical.  The swapped inputs are the events of both samples and the four tables; the reads' layout (offsets, bases,
    starts) is host data the pivot copies itself and stays.  The decoy: the events of each sample end to end, the tables moved."""
    reads1, model, alt, _ = RL.chain_inputs(n_reads=40, shift_sd=2.0)
    canon, _, _, _ = RL.chain_inputs(n_reads=80, shift_sd=0.0)
    reads = (_take_reads(canon, 40, 80), reads1)
    real = dict(val0=reads[0]['norm_mean'].copy(), val1=reads[1]['norm_mean'].copy(), mean=model['mean'].copy(), sd=model['sd'].copy(),
                alt_mean=alt['mean'].copy(), alt_sd=alt['sd'].copy())
    decoy = dict(val0=real['val0'][::-1].copy(), val1=real['val1'][::-1].copy(), mean=real['mean'] + 0.05, sd=real['sd'] * 1.1,
                 alt_mean=real['alt_mean'] - 0.05, alt_sd=real['alt_sd'] * 0.9)
    return dict(real=_frozen(real), decoy=_frozen(decoy), reads=reads, k=model['k'], center=model['center'])
