"""-m gpu: where and when the NMOD_MEM_DEVICE entries run.  include/nanomod_hip.h promises for nmod_fdr_adjust, nmod_mix_fraction,
nmod_one_sample, nmod_kmer_model, nmod_rescale_reads, nmod_read_calls, nmod_site_calls, nmod_read_llr, nmod_site_llr, nmod_site_stoich,
nmod_site_diff and nmod_combine_track, and for nmod_detect_batch outside its three exceptions, that everything is enqueued on
prm->stream with no host read and no synchronisation, and that the process-wide state (the scratch pool, the per-device caches) is
thread-safe and never affects a result.  The method — a bounded stall first, the inputs put in place behind it, a decoy written
behind the call — is described in tests/stream_cases.py, which also records the measured call times the stall is sized from.

Each test prints nothing and reads nothing but plain streams and events: no graph is captured and no queue setting is touched."""
import threading

import numpy as np
import pytest

import stream_cases as S
from test_engine_device_args_gpu import same

pytestmark = pytest.mark.gpu

NAMES = [b.name for b in S.BUILDERS]
# Streams share hardware queues (four by default): work an entry misplaces on a stream that happens to share the stalled stream's queue
# is queued behind the stall after all and stays hidden.  Streams made one after the other take different queues, so every stalled
# case runs on two of them.
STREAMS_TRIED = 2


class Env:
    """one detector; per builder and part the swapped inputs, the outputs of a first (warming) call and the serial result, made once"""

    def __init__(self):
        import torch
        from nanomod_amd import engine
        self.torch, self.engine = torch, engine
        self.det = engine.DeviceDetector(0)                               # stouffer, nb = 2, weights_dif = 2.0, all tests
        self._cases = {}

    def numpy(self, res):
        return {k: v.cpu().numpy() for k, v in res.items()}

    def like(self, res):
        """uninitialised tensors of the shapes of `res`, allocated on the current stream"""
        return {k: self.torch.empty_like(v) for k, v in res.items()}

    def serial(self, call, sw, det=None):
        """step 1 on the current stream: the entry on `real` into outputs that held the sentinel -> (the outputs as numpy, a template of
        them); the inputs are left holding the decoy"""
        torch = self.torch
        sw.load_real()
        first = call(det or self.det, sw.t)                               # fresh outputs: their shapes; loads every kernel
        torch.cuda.synchronize()
        want = self.numpy(call(det or self.det, sw.t, S.fill_sentinel(self.like(first))))
        sw.load_decoy()
        torch.cuda.synchronize()
        return want, first

    def case(self, name, part=1):
        if (name, part) not in self._cases:
            b = S.BY_NAME[name]
            d = b.make_inputs(part)
            sw = S.Swapped(d['real'], d['decoy'])
            want, first = self.serial(b.call, sw)
            self._cases[name, part] = (b, sw, want, first)
        return self._cases[name, part]

    def fresh_stream(self):
        """a new non-blocking stream whose allocator pool already holds a block: nothing a test allocates on it goes to the driver"""
        torch = self.torch
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            warm = [torch.empty(1 << 20, dtype=torch.uint8, device='cuda:0'), torch.empty(8 << 20, dtype=torch.uint8, device='cuda:0')]
        del warm
        s.synchronize()
        return s


@pytest.fixture(scope='module')
def env():
    return Env()


def assert_same_outputs(got, want, what):
    assert set(got) == set(want), what
    bad = [k for k in want if not same(got[k], want[k])]
    assert not bad, (what, bad)


def stalled(env, sw, body, ms, probe_inside=None):
    """Steps 2 and 3: on a fresh stream a stall of `ms`, an event, the real inputs, body() and the decoy behind it.  Returns (what body
    returned, whether the event had completed when the last enqueue returned, the stream — not yet synchronised).  probe_inside: body
    takes a callable and calls it where its non-synchronising stages end; the event is queried there instead."""
    torch = env.torch
    stream = env.fresh_stream()
    seen = []
    with torch.cuda.stream(stream):
        S.stall(stream, ms)
        event = torch.cuda.Event()
        event.record(stream)
        sw.load_real()
        if probe_inside:
            res = body(lambda: seen.append(event.query()))
            sw.load_decoy()
        else:
            res = body()
            sw.load_decoy()
            seen.append(event.query())
    assert len(seen) == 1
    return res, seen[0], stream


# ------------------------------------------------------------------------------------------------- every entry on its own
@pytest.mark.parametrize('name', NAMES)
def test_entry_runs_on_its_stream_and_waits_for_nothing(env, name):
    torch = env.torch
    b, sw, want, first = env.case(name)
    out = env.like(first)                                                 # allocated before the stall, filled behind it
    for _ in range(STREAMS_TRIED):
        got, early, stream = stalled(env, sw, lambda: b.call(env.det, sw.t, S.fill_sentinel(out)), S.T_MS)
        # step 3: the stall had not ended when the call (and the copy behind it) returned: the entry waited for nothing on the stream
        # and read nothing back from it
        assert not early, '%s: the stall of %g ms had ended when the call returned' % (name, S.T_MS)
        stream.synchronize()
        # step 4: whatever ran off the stream, or later than the call's place in it, saw the decoy or the sentinel
        assert_same_outputs(env.numpy(got), want, name)
        assert sw.holds('decoy'), name + ': the inputs were written after the trailing copy, or the copy did not run'


@pytest.mark.parametrize('name', NAMES)
def test_two_calls_in_a_row_wait_for_nothing(env, name):
    """The same entry twice behind one stall: the second call takes scratch of the size the first has just given back while none of it
    has run.  (Found with this file: hipFreeAsync of a block the pool handed out again while its previous free was still queued waited
    on the host for the whole stall; the entries now park their slab per stream, nanomod_amd/csrc/scratch_pool.hpp.)"""
    torch = env.torch
    b, sw, want, first = env.case(name)
    outs = [env.like(first), env.like(first)]
    got, early, stream = stalled(env, sw, lambda: [b.call(env.det, sw.t, S.fill_sentinel(o)) for o in outs], S.T_MS)
    assert not early, '%s: the second call in a row waited for the first' % name
    stream.synchronize()
    for g in got:
        assert_same_outputs(env.numpy(g), want, name)
    assert sw.holds('decoy')


def test_trim_returns_the_parked_slabs(env):
    """nmod_trim_scratch gives back what the calls above left parked per stream, and the entries work on afterwards"""
    torch = env.torch
    lib = env.det.lib
    b, sw, want, first = env.case('site_stoich')
    torch.cuda.synchronize()
    held = torch.cuda.mem_get_info(0)[0]
    assert lib.nmod_trim_scratch(0) == 0
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info(0)[0] >= held
    sw.load_real()
    assert_same_outputs(env.numpy(b.call(env.det, sw.t, S.fill_sentinel(env.like(first)))), want, 'after the trim')
    sw.load_decoy()
    torch.cuda.synchronize()
    assert lib.nmod_trim_scratch(0) == 0 and lib.nmod_trim_scratch(0) == 0


@pytest.mark.parametrize('name', NAMES)
def test_the_decoy_gives_other_results(env, name):
    """what step 4 rests on: the entry run on the decoy does not give the results of the real batch"""
    b, sw, want, first = env.case(name)
    assert sw.holds('decoy')
    other = env.numpy(b.call(env.det, sw.t, S.fill_sentinel(env.like(first))))
    changed = [k for k in want if not same(other[k], want[k])]
    assert len(changed) * 2 >= len(want), (name, changed)                 # most outputs differ, not one status word


# ------------------------------------------------------------------------------------------------------------ the pipelines
def _chain1(env, det, t, out=None):
    """det.run -> det.fdr -> det.mix(gate = q): tests, q-values and the fractions of the rejected positions as one stream"""
    o = out or {}
    res = S.run_call(det, t, o.get('run'))
    (q,), summary = det.fdr(res, tracks=('comb_p',), method='bh', alpha=S.RUN_ALPHA, out=o.get('fdr'))
    mix = det.mix(t['sig0'], t['sig1'], off0=t['off0'], off1=t['off1'], gate=q, gate_max=S.RUN_ALPHA, max_iter=40, out=o.get('mix'))
    return dict(run=res, fdr={'comb_p': q}, mix=mix, summary={'summary': summary})


def _flatten(parts):
    return {a + '.' + k: v for a, res in parts.items() for k, v in res.items()}


def test_chain_detect_fdr_mix_as_one_stream(env):
    torch = env.torch
    d = S.run_inputs(1)
    sw = S.Swapped(d['real'], d['decoy'])
    sw.load_real()
    first = _chain1(env, env.det, sw.t)
    torch.cuda.synchronize()
    template = lambda: {k: S.fill_sentinel(env.like(first[k])) for k in ('run', 'fdr', 'mix')}
    want = env.numpy(_flatten(_chain1(env, env.det, sw.t, template())))
    torch.cuda.synchronize()
    status = want['mix.status']
    assert 0 < int((status & 4).astype(bool).sum()) < len(status)         # the q-values gate some positions off and let some through
    outs = {k: env.like(first[k]) for k in ('run', 'fdr', 'mix')}         # allocated before the stall
    for _ in range(STREAMS_TRIED):
        got, early, stream = stalled(env, sw, lambda: _chain1(env, env.det, sw.t, {k: S.fill_sentinel(v) for k, v in outs.items()}), S.T_MS)
        assert not early, 'a stage of run -> fdr -> mix waited for the stream'
        stream.synchronize()
        assert_same_outputs(env.numpy(_flatten(got)), want, 'run -> fdr -> mix')
        assert sw.holds('decoy')


def _chain2(env, det, c, t, probe=None):
    """rescale_reads -> read_llr for both samples (nothing synchronises: probe() is called behind them), then pivot_reads(val = llr_win)
    for both -> match_score_rows -> site_diff -> fdr: the pivot and the matching synchronise by contract"""
    engine = env.engine
    k, center = c['k'], c['center']
    names = engine.chrom_names(*c['reads'])
    llr = []
    for s in (0, 1):
        off, base = c['dev'][s]
        r = det.rescale_reads(t['val%d' % s], off, base, t['mean'], t['sd'], k, center)
        llr.append(det.read_llr(r['val'], off, base, t['mean'], t['sd'], t['alt_mean'], t['alt_sd'], k, center, want=('llr_win',)))
    if probe:
        probe()
    g = [engine.pivot_reads(c['reads'][s], val=llr[s]['llr_win'], names=names) for s in (0, 1)]
    m = engine.match_score_rows(g[0], g[1], S.CHAIN_MIN_COVERAGE)
    diff = det.site_diff(m['sig0'], m['sig1'], off0=m['off0'], off1=m['off1'])
    (q,), summary = det.fdr(diff, tracks=('p_diff',))
    res = dict(diff, q=q, summary=summary, key=m['key'], off0=m['off0'], off1=m['off1'])
    res.update({'llr_win%d' % s: llr[s]['llr_win'] for s in (0, 1)})
    return res


def test_chain_rescale_llr_pivot_diff_fdr_as_one_stream(env):
    torch = env.torch
    c = dict(S.chain2_inputs())
    dev = lambda a: torch.from_numpy(np.array(a, order='C')).to('cuda:0')
    c['dev'] = [(dev(r['off']), dev(np.asarray(r['base']).astype('S1').view(np.uint8))) for r in c['reads']]
    sw = S.Swapped(c['real'], c['decoy'])
    sw.load_real()
    want = env.numpy(_chain2(env, env.det, c, sw.t))
    torch.cuda.synchronize()
    assert len(want['key']) > 100 and np.nanmin(want['p_diff']) < 1e-3    # the planted site is there to be found
    for _ in range(STREAMS_TRIED):
        got, early, stream = stalled(env, sw, lambda probe: _chain2(env, env.det, c, sw.t, probe), S.T_MS, probe_inside=True)
        assert not early, 'rescale_reads or read_llr waited for the stream'
        stream.synchronize()
        assert_same_outputs(env.numpy(got), want, 'rescale -> llr -> pivot -> match -> diff -> fdr')
        assert sw.holds('decoy')


# ----------------------------------------------------------------------------------- entries that synchronise by contract
def test_argsort_device_orders_against_its_stream(env):
    """nmod_argsort_keys with device inputs synchronises before returning; its work still belongs on prm->stream: steps 2 and 4"""
    rng = np.random.default_rng(171)
    n = 50000
    sw = S.Swapped({'key': rng.integers(-1000, 1000, n)}, {'key': rng.integers(-(1 << 40), 1 << 40, n)})
    sw.load_real()
    want = env.engine.argsort_device(sw.t['key']).cpu().numpy()
    assert np.array_equal(want, np.argsort(sw.real['key'].cpu().numpy(), kind='stable'))
    for _ in range(STREAMS_TRIED):
        got, _, stream = stalled(env, sw, lambda: env.engine.argsort_device(sw.t['key']), S.SHORT_STALL_MS)
        stream.synchronize()
        assert same(got.cpu().numpy(), want) and sw.holds('decoy')


def test_pivot_reads_orders_against_its_stream(env):
    """nmod_pivot_reads synchronises its stream a few times by contract; the events it is given as a device tensor are read on that
    stream, behind whatever produced them: steps 2 and 4"""
    c = S.chain2_inputs()
    reads = c['reads'][1]
    rng = np.random.default_rng(172)
    nev = int(reads['off'][-1])
    sw = S.Swapped({'val': rng.normal(0.0, 3.0, nev)}, {'val': rng.normal(0.0, 3.0, nev)})
    fields = ('key', 'off', 'sig', 'base')
    sw.load_real()
    want = env.numpy({k: v for k, v in env.engine.pivot_reads(reads, val=sw.t['val']).items() if k in fields})
    assert len(want['key']) > 100 and len(want['sig']) == nev
    for _ in range(STREAMS_TRIED):
        got, _, stream = stalled(env, sw, lambda: env.engine.pivot_reads(reads, val=sw.t['val']), S.SHORT_STALL_MS)
        stream.synchronize()
        assert_same_outputs(env.numpy({k: v for k, v in got.items() if k in fields}), want, 'pivot_reads')
        assert sw.holds('decoy')


# ------------------------------------------------------------------------------------------------ two threads, two streams
THREAD_ROUNDS = 4


def _thread_cases(env, names):
    """for both threads, every builder of `names` and both sizes: inputs of the thread's own holding the real batch, and the serial result"""
    torch = env.torch
    cases = {}
    for name in names:
        for part in (1, 3):
            b, _, want, _ = env.case(name, part)
            d = b.make_inputs(part)
            for who in (0, 1):
                sw = S.Swapped(d['real'], d['decoy'])
                sw.load_real()
                cases[who, name, part] = (b, sw, want)
    torch.cuda.synchronize()
    return cases


def _walk(env, cases, who, names, stream, errors):
    """THREAD_ROUNDS times over `names` on the thread's own stream and detector, the batch sizes alternating between the builder's size
    and about a third of it: slabs of different sizes pass between the two streams through the library's pool"""
    torch = env.torch
    try:
        det = env.engine.DeviceDetector(0)
        with torch.cuda.stream(stream):
            for rnd in range(THREAD_ROUNDS):
                for i, name in enumerate(names):
                    part = (1, 3)[(rnd + i + who) % 2]
                    b, sw, want = cases[who, name, part]
                    got = env.numpy(b.call(det, sw.t))
                    bad = [k for k in want if not same(got[k], want[k])]
                    if bad or set(got) != set(want):
                        errors.append((who, name, part, rnd, bad))
    except Exception as e:                                                # noqa: BLE001 — reported by the caller
        errors.append((who, repr(e)))


def test_two_threads_two_streams_walk_the_twelve_entries(env):
    torch = env.torch
    names = [b.name for b in S.ENTRY_BUILDERS]
    cases = _thread_cases(env, names)
    errors = []
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    th = [threading.Thread(target=_walk, args=(env, cases, 0, names, streams[0], errors)),
          threading.Thread(target=_walk, args=(env, cases, 1, names[::-1], streams[1], errors))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


def test_kernel_entries_beside_the_host_pipeline(env):
    """thread A walks K8 .. K15 on its stream while thread B runs nmod_detect_batch on host memory: the pipelined host entry with its
    own streams and pinned ring, cut into many chunks"""
    import nanomod_amd as nm
    torch = env.torch
    lib = nm._lib.load()
    names = list(S.KERNEL_ENTRIES)
    cases = _thread_cases(env, names)
    r = S.run_inputs(1)['real']
    host = lambda: nm.detect_host(r['sig0'], r['off0'], r['sig1'], r['off1'], r['run_id'], nb=2, weights_dif=2.0, method='stouffer', tests=7)
    assert lib.nmod_host_pipeline_config(64 << 10, 3, 2, 0) == 0          # many chunks per call
    try:
        want = host()
        device_want = env.case('detect_batch')[2]
        assert all(same(want[k], device_want[k]) for k in want)           # the two memspaces agree on this batch
        errors = []

        def host_worker():
            try:
                for rnd in range(THREAD_ROUNDS):
                    got = host()
                    if not all(same(got[k], want[k]) for k in want):
                        errors.append(('host', rnd))
            except Exception as e:                                        # noqa: BLE001
                errors.append(('host', repr(e)))
        th = [threading.Thread(target=_walk, args=(env, cases, 0, names, torch.cuda.Stream(), errors)), threading.Thread(target=host_worker)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errors, errors
    finally:
        lib.nmod_host_pipeline_config(0, 0, 0, 0)
