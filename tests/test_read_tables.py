"""The text tables of the read-level pipelines (readcalls, rescale, readllr: twenty writers) byte for byte, and the refusals of the
pipelines' shared set-up before any device work.

Every writer gets one small table built by hand — a '-' strand row, a position 0, a row with NaN in every float column that can hold
one — with and without its optional column, and the empty table.  tests/golden/read_tables/expected.json holds the files the writers
of commit e815bed (the last one in which every writer built its own columns) wrote for the same tables."""
import json
import os

import numpy as np
import pytest

from nanomod_amd import readcalls as RC
from nanomod_amd import readllr as RL
from nanomod_amd import rescale as RS

EXPECTED = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'read_tables', 'expected.json')
NAN = float('nan')

_HEAD = dict(chrom=np.array(['chr1', 'chr1', 'chrM', 'chr2']), strand=np.array(['+', '-', '+', '-']))
_SITE = dict(_HEAD, pos=np.array([0, 41, 1234567, 7], np.int64), base=np.array(['A', 'c', 'N', 'T']))
_READ = dict(_HEAD, index=np.arange(4, dtype=np.int64), start=np.array([0, 5, 99999, 12], np.int64), events=np.array([300, 1, 0, 47], np.int64))
_F = lambda *v: np.array(v, np.float64)
_I = lambda *v: np.array(v, np.int32)
_U8 = lambda *v: np.array(v, np.uint8)


def _without(d, *keys):
    return {k: v for k, v in d.items() if k not in keys}


def _cut(x):
    """the empty table of a table: every array and list without its entries, scalars as they are"""
    if isinstance(x, dict):
        return {k: _cut(v) for k, v in x.items()}
    if isinstance(x, np.ndarray):
        return x[:0]
    return [] if isinstance(x, list) else x


def _site_diff_rep(G):
    nv = np.arange(4 * G, dtype=np.int32).reshape(4, G)
    ps = np.linspace(0.0, 1.0, 4 * G).reshape(4, G)
    ps[2] = NAN
    return dict(_SITE, n_samples=G, n_control=G // 2, n_valid=nv, pi_s=ps, pi0=_F(0.1, 0.25, NAN, 0.0), pi1=_F(0.9, 0.5, NAN, 1.0),
                pi_pool=_F(0.5, 0.375, NAN, 0.5), delta=_F(0.8, 0.25, NAN, 1.0), delta_lo=_F(0.7, -0.1, NAN, 0.123456789),
                delta_hi=_F(0.9, 0.6, NAN, 1.0), stat_cond=_F(30.1234, 2.0, NAN, 0.0), p_cond=_F(1.5e-8, 0.157, NAN, 1.0),
                stat_het=_F(1.0005, 0.0, NAN, 7.25), p_het=_F(0.6, 1.0, NAN, 2.5e-300), phi=_F(1.0, 0.5, NAN, 12.3456), p_rep=_F(3e-5, 0.2, NAN, 0.0),
                q=_F(6e-5, 0.4, NAN, 0.0), rep_status=_U8(0, 4, 1, 255))


def _tables():
    """case name -> (writer, arguments after the path)"""
    read_calls = dict(_READ, n_sites=_I(290, 1, 0, 40), n_called=_I(3, 0, 0, 40), status=_U8(0, 0, 1, 0))
    site_calls = dict(_SITE, n_reads=_I(10, 3, 1, 200), n_valid=_I(9, 3, 0, 200), n_called=_I(2, 0, 0, 200), frac=_F(2 / 9, 0.0, NAN, 1.0))
    scale = dict(_READ, n_used=_I(280, 0, 0, 45), shift=_F(0.0123456, -1.5, NAN, 0.0), scale=_F(1.0000004, 0.5, NAN, 2.0), status=_U8(0, 1, 2, 16))
    scale_reads = dict(chrom=np.array(['a', 'b', 'c', 'd']), strand=np.array(['-', '-', '+', '+']), start=np.array([9, 8, 0, 6], np.int64))
    read_llr = dict(_READ, n_sites=_I(290, 1, 0, 40), n_mod=_I(3, 0, 0, 20), n_can=_I(200, 1, 0, 20), status=_U8(0, 0, 1, 0))
    site_llr = dict(_SITE, n_reads=_I(10, 3, 1, 200), n_valid=_I(9, 3, 0, 200), n_mod=_I(2, 0, 0, 100), n_can=_I(6, 0, 0, 100),
                    frac=_F(0.25, NAN, NAN, 0.5))
    stoich = dict(site_llr, pi=_F(0.2500004, 0.0, NAN, 1.0), pi_lo=_F(0.1, 0.0, NAN, 0.9999995), pi_hi=_F(0.4, 0.3, NAN, 1.0),
                  stat=_F(12.3456, 0.0, NAN, 1e4), p_null=_F(4.4e-4, 1.0, NAN, 0.0), stoich_status=_U8(0, 2, 1, 0))
    diff = dict(_SITE, n_reads0=_I(10, 5, 1, 60), n_reads1=_I(12, 5, 2, 61), n_valid0=_I(9, 5, 0, 60), n_valid1=_I(12, 4, 1, 61),
                pi0=_F(0.1, 0.25, NAN, 0.0), pi1=_F(0.9, 0.5, NAN, 1.0), pi_pool=_F(0.5, 0.375, NAN, 0.5), delta=_F(0.8, 0.25, NAN, 1.0),
                delta_lo=_F(0.7, -0.1, NAN, 0.123456789), delta_hi=_F(0.9, 0.6, NAN, 1.0), stat=_F(30.1234, 2.0, NAN, 0.0),
                p_diff=_F(1.5e-8, 0.157, NAN, 1.0), q=_F(6e-8, 0.3, NAN, 1.0), diff_status=_U8(0, 4, 1, 255))
    pair_head = dict(_HEAD, pos_a=np.array([0, 41, 1234567, 7], np.int64), pos_b=np.array([1, 141, 1234570, 50], np.int64),
                     dist=np.array([1, 100, 3, 43], np.int64))
    pairs = dict(pair_head, n11=_I(10, 0, 0, 5), n10=_I(1, 2, 0, 5), n01=_I(2, 3, 0, 5), n00=_I(20, 4, 0, 5),
                 log_or=_F(4.123456789, -1.0, NAN, 0.0), se=_F(0.9, 1.5, NAN, 0.894427191), phi=_F(0.7, -0.2, NAN, 0.0),
                 p_fisher=_F(1e-5, 0.5, NAN, 1.0), q=_F(4e-5, 0.75, NAN, 1.0), status=_U8(0, 0, 1, 0))
    link = dict(pair_head, n_cov=_I(40, 20, 3, 25), pa=_F(0.3, 0.5, NAN, 1e-9), pb=_F(0.35, 0.5, NAN, 0.5), d=_F(0.2, 0.0, NAN, -1e-7),
                d_lo=_F(0.1, -0.1, NAN, -0.25), d_hi=_F(0.25, 0.1, NAN, 0.25), r=_F(0.9, 0.0, NAN, -0.5), pi11=_F(0.305, 0.25, NAN, 0.0),
                pi10=_F(-0.005, 0.25, NAN, 0.0), pi01=_F(0.045, 0.25, NAN, 0.5), pi00=_F(0.655, 0.25, NAN, 0.5), stat=_F(20.5, 0.0, NAN, 0.0005),
                p_indep=_F(6e-6, 1.0, NAN, 0.98), q_indep=_F(2.4e-5, 1.0, NAN, 0.98), link_status=_U8(0, 0, 1, 2))
    fit = dict(trace=[(0.3, 200.0, -1234.5678901, 12.5), (0.25, 150.123456789, -1230.0, 1e-12)], pi=0.25, pi_lo=0.2, pi_hi=0.30000000004,
               se_eta=0.12345678, length=150.123456789, length_lo=150.123456789, length_hi=150.123456789, se_lam=NAN, n_eval=5, converged=True,
               ci_level=0.95, status='pi fitted alone: no read has two entries, length is not identified')
    hmm_reads = dict(_without(_READ, 'start', 'events'), n_sites=_I(12, 0, 3, 1), n_mod=_I(4, 0, 0, 1), n_can=_I(6, 0, 3, 0), n_runs=_I(2, 0, 0, 1),
                     ll=_F(-10.5, 0.0, NAN, -0.6931471805599453), ll_indep=_F(-12.25, 0.0, NAN, -0.6931471805599453), status=_U8(0, 1, 0, 0))
    hmm_sites = dict(_without(_SITE, 'base'), n=_I(10, 3, 0, 7), n_mod=_I(4, 0, 0, 7), n_can=_I(5, 0, 0, 0), share=_F(4 / 9, NAN, NAN, 1.0))
    domains = dict(read=np.array([0, 0, 3, 1], np.int64), first=np.array([0, 30, 7, 41], np.int64), last=np.array([12, 30, 1234567, 41], np.int64),
                   n_sites=np.array([3, 1, 9, 1], np.int64), mean_post=_F(0.95, 0.9000004, NAN, 1.0), min_delta=_F(2.5, 0.0, NAN, 1e-7))
    hmm = dict(reads=hmm_reads, sites=hmm_sites, domains=_without(domains, 'min_delta'),
               site_prior=dict(_without(_SITE, 'base'), n_valid=_I(40, 2, 0, 7), pi_hat=_F(0.25, 1.0, NAN, 1 / 3), prior=_F(0.2727272727272727, 0.5, NAN, 0.4)))
    vit = dict(reads=_without(hmm_reads, 'n_can', 'll', 'll_indep'), domains=domains,
               sites=dict(_without(hmm_sites, 'n_can', 'share'), share=_F(0.4, 0.0, NAN, 1.0)),
               entries=dict(hoff=np.array([0, 2, 2, 3, 4], np.int64), site=np.array([0, 3, 1, 2], np.int32), path=_U8(1, 0, 0, 1),
                            delta=_F(3.25, -0.0000004, NAN, 0.0)))
    classes = dict(C=2, reads=dict(_without(_READ, 'start', 'events'), n_sites=_I(12, 0, 3, 1), cls=_I(0, -1, 1, 0), gamma=_F(0.99, 0.0, NAN, 0.5),
                                   ll=_F(-10.5, 0.0, NAN, -0.6931471805599453)),
                   sites=dict(_without(_SITE, 'base'), theta=np.array([[0.9, 0.1], [0.5, 0.5], [NAN, NAN], [1e-9, 1.0 - 1e-9]]),
                              n=np.array([[30.25, 12.0], [0.0, 0.0004], [NAN, NAN], [5.0, 1000.0]])),
                   fit=[dict(C=1, start=0, w=(1.0,), ll=-2000.123456, bic=4010.5, n_iter=2, converged=True, kept=True),
                        dict(C=2, start=0, w=(0.6000004, 0.3999996), ll=-1900.0, bic=3820.25, n_iter=500, converged=False, kept=False),
                        dict(C=2, start=1, w=(0.75, 0.25), ll=NAN, bic=float('inf'), n_iter=17, converged=True, kept=True)])
    cases = {
        'read_calls': (RC.write_read_calls, (read_calls,)), 'site_calls': (RC.write_site_calls, (site_calls,)),
        'read_scale_from_table': (RS.write_read_scale, (None, scale)), 'read_scale_from_reads': (RS.write_read_scale, (scale_reads, scale)),
        'read_llr': (RL.write_read_llr, (read_llr,)), 'site_llr': (RL.write_site_llr, (site_llr,)), 'site_stoich': (RL.write_site_stoich, (stoich,)),
        'site_diff_q': (RL.write_site_diff, (diff,)), 'site_diff': (RL.write_site_diff, (_without(diff, 'q'),)),
        'site_diff_rep_g3_q': (RL.write_site_diff_rep, (_site_diff_rep(3),)), 'site_diff_rep_g3': (RL.write_site_diff_rep, (_without(_site_diff_rep(3), 'q'),)),
        'site_diff_rep_g4_q': (RL.write_site_diff_rep, (_site_diff_rep(4),)), 'site_diff_rep_g4': (RL.write_site_diff_rep, (_without(_site_diff_rep(4), 'q'),)),
        'site_pairs_q': (RL.write_site_pairs, (pairs,)), 'site_pairs': (RL.write_site_pairs, (_without(pairs, 'q'),)),
        'site_linkage_q': (RL.write_site_linkage, (link,)), 'site_linkage': (RL.write_site_linkage, (_without(link, 'q_indep'),)),
        'hmm_fit': (RL.write_hmm_fit, (fit,)), 'read_hmm': (RL.write_read_hmm, (hmm,)), 'read_domains': (RL.write_read_domains, (hmm,)),
        'read_domains_min_delta': (RL.write_read_domains, (vit,)), 'site_hmm': (RL.write_site_hmm, (hmm,)),
        'read_viterbi': (RL.write_read_viterbi, (vit,)), 'site_prior': (RL.write_site_prior, (hmm,)), 'site_viterbi': (RL.write_site_viterbi, (vit,)),
        'read_classes': (RL.write_read_classes, (classes,)), 'class_sites': (RL.write_class_sites, (classes,)),
        'classes_fit': (RL.write_classes_fit, (classes,)),
    }
    for name, (write, args) in list(cases.items()):
        cases[name + '_empty'] = (write, tuple(_cut(a) for a in args))
    return cases


CASES = _tables()


def written(name, folder):
    write, args = CASES[name]
    path = os.path.join(str(folder), name + '.txt')
    write(path, *args)
    with open(path, 'rb') as f:
        return f.read()


@pytest.fixture(scope='module')
def expected():
    with open(EXPECTED) as f:
        return json.load(f)


def test_every_writer_has_a_case_and_every_case_a_record(expected):
    writers = {getattr(m, n) for m in (RC, RS, RL) for n in dir(m) if n.startswith('write_') and getattr(m, n).__module__ == m.__name__}
    assert len(writers) == 20 and {w for w, _ in CASES.values()} == writers
    assert sorted(expected) == sorted(CASES)


@pytest.mark.parametrize('name', sorted(CASES))
def test_writer_bytes_are_the_recorded_ones(name, expected, tmp_path):
    assert written(name, tmp_path) == expected[name].encode('ascii')


# ------------------------------------------------------------------------------------- the shared set-up refuses before the device
@pytest.fixture
def no_device(monkeypatch):
    """any step towards the device fails the test"""
    from nanomod_amd import engine

    def reached(*a, **kw):
        raise AssertionError('device work before the refusal')
    monkeypatch.setattr(engine, '_join_warm_up', reached)
    monkeypatch.setattr(engine, 'DeviceDetector', reached)


_RESCALE_MSG = 'rescale: unknown option(s) level; known: weighted, clip_sigma, clip_rounds, min_events, scale_range'
_K_MSG = 'the two models must share k and center: 3 / 0 and 3 / 1'
_PRIOR_MSG = 'prior must lie inside (0, 1)'
_WINDOW_MSG = "window must be 'kmer' or (lo, hi)"
# (keywords, alt model's center, the refusal): each inline copy's refusals one by one, then two at a time: the earlier one wins
_SETUP_REFUSALS = (
    (dict(), 1, _K_MSG), (dict(prior=0.0), 0, _PRIOR_MSG), (dict(prior=1.0), 0, _PRIOR_MSG), (dict(rescale=dict(level=1)), 0, _RESCALE_MSG),
    (dict(window='wide'), 0, _WINDOW_MSG), (dict(window=(1, 2, 3)), 0, _WINDOW_MSG), (dict(window=(0, 1 << 20)), 0, 'the window bounds must be in 0 .. 64'),
    (dict(prior=2.0), 1, _K_MSG), (dict(prior=2.0, rescale=dict(level=1)), 0, _PRIOR_MSG), (dict(rescale=dict(level=1), window='wide'), 0, _RESCALE_MSG),
)


@pytest.mark.parametrize('entry', ['call_reads_llr', 'compare_reads_llr', 'compare_reads_llr_rep'])
def test_shared_setup_refuses_with_the_same_text_before_any_device_work(entry, no_device):
    import readllr_ref as RF
    from nanomod_amd import _lib as L
    assert L.MAX_NB == 64
    reads, model, alt, _ = RF.chain_inputs(n_reads=4, shift_sd=2.0)
    lead = {'call_reads_llr': (reads,), 'compare_reads_llr': (reads, reads), 'compare_reads_llr_rep': ([reads, reads], [reads])}[entry]
    later = dict(stoich=dict(level=1)) if entry == 'call_reads_llr' else dict(diff=dict(level=1), min_coverage=0)
    for kw, center, msg in _SETUP_REFUSALS:
        for more in ({}, later):                                                          # a later refusal does not come first
            with pytest.raises(ValueError) as e:
                getattr(RL, entry)(*lead, model, dict(alt, center=center), log=None, **kw, **more)
            assert str(e.value) == msg, (kw, more)
    # ... and a set that is no read-level set is refused after the set-up, with _checked_reads' text
    position_set = dict(pos=np.arange(3), norm_mean=np.zeros(3, np.float32))
    lead = {'call_reads_llr': (position_set,), 'compare_reads_llr': (reads, position_set), 'compare_reads_llr_rep': ([reads, reads], [position_set])}[entry]
    which = {'call_reads_llr': 'reads', 'compare_reads_llr': 'reads1', 'compare_reads_llr_rep': 'reads1[0]'}[entry]
    with pytest.raises(ValueError) as e:
        getattr(RL, entry)(*lead, model, alt, log=None)
    assert str(e.value) == which + ' is not a read-level set (no chrom, strand, start, off, base): per-position containers have no reads'
    with pytest.raises(ValueError) as e:
        getattr(RL, entry)(*lead, model, alt, log=None, window='wide')
    assert str(e.value) == _WINDOW_MSG


def test_call_reads_refuses_a_set_without_reads_with_a_message(no_device):
    """call_reads and call_reads_llr take their arrays from _checked_reads: a per-position container is a ValueError that says so (it was
    a bare KeyError), still before any device work and still after the refusal of an unknown rescale option"""
    import readllr_ref as RF
    _, model, alt, _ = RF.chain_inputs(n_reads=4, shift_sd=2.0)
    position_set = dict(pos=np.arange(3), norm_mean=np.zeros(3, np.float32))
    with pytest.raises(ValueError) as e:
        RC.call_reads(position_set, model, log=None)
    assert str(e.value) == 'reads is not a read-level set (no chrom, strand, start, off, base): per-position containers have no reads'
    with pytest.raises(ValueError) as e:
        RC.call_reads(position_set, model, rescale=dict(level=1), log=None)
    assert str(e.value) == _RESCALE_MSG
