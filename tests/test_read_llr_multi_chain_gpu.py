"""The chain of K26 through the Python layers and the command line on a seeded planted set (multi_ref.chain_inputs: 240 reads over one
short reference, three sites that hold state 1, state 2 and neither): call_reads_llr_multi and `cli readllr` with two --altModel paths find
each planted state at its site, the counts add up, the --fdr column is there; and with ONE --altModel path the three files the command
has always written are byte for byte what the same command wrote before K26 (their hashes recorded from the parent commit's build)."""
import hashlib
import os

import numpy as np
import pytest

import multi_ref as M
from nanomod_amd import _lib as L, engine, multimod
from nanomod_amd import readllr as RL

pytestmark = pytest.mark.gpu

NAMES = ['m6A', 'm5C']

# sha256 of <FileID>_read_llr.txt, _site_llr.txt and _site_stoich.txt of single_alt_argv() below, written by the parent commit's build
# (the commit before K26) on an MI355X
PARENT_SHA256 = {
    'one_read_llr.txt': '333c13bc6ecbb467fc29dcaaed03f43b0f5584da9b2143f549a6fc5d90fd4f40',
    'one_site_llr.txt': '60ef67c5d92b9fa927393507070b2f357eb049af121d54392ceb869a611cbc92',
    'one_site_stoich.txt': '4451d415be2ca476fe2e80d53ee3ee1c5e86778a68e6972dbc534338927e89ca',
}


def write_inputs(tmp):
    """the planted set as files: (reads path, model path, the two alternative model paths)"""
    from nanomod_amd import container, kmermodel
    reads, model, alts, sites = M.chain_inputs()
    paths = [os.path.join(str(tmp), n) for n in ('reads.npz', 'model.npz', 'alt1.npz', 'alt2.npz')]
    container.save_reads(paths[0], *[reads[f] for f in ('chrom', 'strand', 'start', 'off', 'norm_mean', 'base')])
    zeros = np.zeros(64, np.int64)
    for path, m in zip(paths[1:], [model] + alts):
        kmermodel.save_kmer_model(path, dict(version=kmermodel.KMER_MODEL_VERSION, clip_sigma=0.0, k=3, center=0, mean=m['mean'], sd=m['sd'],
                                             n_positions=m['n_positions'], n_samples=zeros + 10, n_clipped=zeros))
    return paths


def single_alt_argv(paths, out):
    """the command of before K26: one --altModel path, the per-site share as well"""
    return ['readllr', '--wrkBase1', paths[0], '--kmerModel', paths[1], '--altModel', paths[2], '--outFolder', out, '--outLevel', '3', '--FileID', 'one',
            '--siteFraction', '1', '--llrThreshold', '2', '--prior', '0.3']


def sha256_of(path):
    with open(path, 'rb') as f:
        return hashlib.sha256(f.read()).hexdigest()


def _at(sites, strand, pos):
    return int(np.flatnonzero((sites['strand'] == strand) & (sites['pos'] == pos))[0])


def _check_planted(sites, planted):
    """at site A state 1 holds the largest share of the two states and is clearly there, at B state 2, at C neither; the hard calls agree"""
    A, B, C = planted
    for strand in '+-':
        a, b, c = (_at(sites, strand, p) for p in (A, B, C))
        assert sites['pi_m6A'][a] > 0.25 and sites['pi_m6A'][a] > 5.0 * sites['pi_m5C'][a] and sites['p_m6A'][a] < 1e-6
        assert sites['pi_m5C'][b] > 0.25 and sites['pi_m5C'][b] > 5.0 * sites['pi_m6A'][b] and sites['p_m5C'][b] < 1e-6
        assert sites['pi_can'][c] > 0.9 and sites['p_m6A'][c] > 1e-3 and sites['p_m5C'][c] > 1e-3
        assert sites['n_m6A'][a] > 5 * max(sites['n_m5C'][a], 1) and sites['n_m5C'][b] > 5 * max(sites['n_m6A'][b], 1)
        assert sites['q_m6A'][a] < 0.05 and sites['q_m5C'][b] < 0.05 and sites['q_m6A'][c] > 0.05


def test_call_reads_llr_multi_finds_the_planted_states():
    reads, model, alts, planted = M.chain_inputs()
    lines = []
    table, sites, ev = RL.call_reads_llr_multi(reads, model, alts, names=NAMES, priors=[0.3, 0.1], compose={}, fdr='bh', events=True, log=lines.append)
    assert len(lines) == 1 and lines[0].startswith('readllr: 240 read(s)') and 'm6A' in lines[0] and 'position(s) with shares' in lines[0]
    assert table['names'] == NAMES == sites['names'] and np.array_equal(table['events'], np.diff(reads['off']))
    amb = np.array([int((ev['call'][a:b] == M.AMBIGUOUS).sum()) for a, b in zip(reads['off'][:-1], reads['off'][1:])])
    assert np.array_equal(table['n_sites'], table['n_can'] + table['n_mod_m6A'] + table['n_mod_m5C'] + amb)
    # the per-site counts are the per-read counts, regrouped: every event lies at one position
    for r, s in (('n_can', 'n_can'), ('n_mod_m6A', 'n_m6A'), ('n_mod_m5C', 'n_m5C'), ('n_sites', 'n_valid')):
        assert int(table[r].sum()) == int(sites[s].sum()), r
    assert int(sites['n_ambiguous'].sum()) == int(amb.sum()) and (sites['n_ambiguous'] >= 0).all()
    # the device chain is the host entry's results
    host = engine.read_llr_multi_host(reads['norm_mean'], reads['off'], reads['base'], model, alts, thr=2.5, prior_logit=multimod._prior_logits([0.3, 0.1], 2))
    assert all(np.ascontiguousarray(ev[f]).tobytes() == host[f].tobytes() for f in L.LLR_MULTI_EVENT_FIELDS)
    assert np.array_equal(table['n_mod_m5C'], host['n_mod'][1]) and np.array_equal(table['n_can'], host['n_can'])
    est = (sites['compose_status'] & L.COMPOSE_NO_ESTIMATE) == 0
    assert est.sum() > 500 and np.allclose((sites['pi_can'] + sites['pi_m6A'] + sites['pi_m5C'])[est], 1.0, atol=1e-12)
    _check_planted(sites, planted)
    with pytest.raises(ValueError):
        RL.call_reads_llr_multi(reads, model, alts, fdr='bh', log=None)
    plain = RL.call_reads_llr_multi(reads, model, alts, log=lambda *a: None)
    assert len(plain) == 2 and 'pi_can' not in plain[1] and np.array_equal(plain[1]['n_mod1'], sites['n_m6A'])


def test_command_line_with_two_alt_models(tmp_path):
    from nanomod_amd import cli, kmermodel
    paths = write_inputs(tmp_path)
    reads, model, alts, planted = M.chain_inputs()
    out = str(tmp_path / 'cli')
    argv = ['readllr', '--wrkBase1', paths[0], '--kmerModel', paths[1], '--altModel', paths[2] + ',' + paths[3], '--outFolder', out, '--outLevel', '3']
    assert cli.main(argv + ['--FileID', 'two', '--modNames', 'm6A,m5C', '--modPrior', '0.3,0.1', '--siteCompose', '1', '--fdr', 'bh']) == 0
    assert sorted(os.listdir(out)) == ['two_read_llr_multi.txt', 'two_site_compose.txt', 'two_site_llr_multi.txt']
    table, sites = RL.call_reads_llr_multi(reads, kmermodel.load_kmer_model(paths[1]), [kmermodel.load_kmer_model(p) for p in paths[2:]], names=NAMES,
                                           priors=[0.3, 0.1], compose=dict(min_valid=3, max_iter=500, tol=1e-9), fdr='bh', log=lambda *a: None)
    t = [ln.split() for ln in open(os.path.join(out, 'two_read_llr_multi.txt')).read().splitlines()]
    assert t[0] == ['#index', 'chrom', 'strand', 'start', 'events', 'n_sites', 'n_can', 'n_mod_m6A', 'n_mod_m5C', 'status'] and len(t) == 241
    for col, f in ((5, 'n_sites'), (6, 'n_can'), (7, 'n_mod_m6A'), (8, 'n_mod_m5C'), (9, 'status')):
        assert [int(r[col]) for r in t[1:]] == table[f].tolist(), f
    u = [ln.split() for ln in open(os.path.join(out, 'two_site_llr_multi.txt')).read().splitlines()]
    assert u[0][-4:] == ['n_can', 'n_m6A', 'n_m5C', 'n_ambiguous'] and len(u) == len(sites['pos']) + 1
    assert [int(r[8]) for r in u[1:]] == sites['n_m5C'].tolist() and [int(r[2]) for r in u[1:]] == (sites['pos'] + 1).tolist()
    c = [ln.split() for ln in open(os.path.join(out, 'two_site_compose.txt')).read().splitlines()]
    head = c[0]
    assert head[7:16] == ['pi_can', 'pi_m6A', 'stat_m6A', 'p_m6A', 'q_m6A', 'pi_m5C', 'stat_m5C', 'p_m5C', 'q_m5C'] and all(len(r) == len(head) for r in c)
    assert [r[head.index('pi_m6A')] for r in c[1:]] == ['%.6f' % v for v in sites['pi_m6A']]
    assert [r[head.index('q_m5C')] for r in c[1:]] == [('%.3E' % v if v == v else 'nan') for v in sites['q_m5C']]
    rows = {(r[1], int(r[2]) - 1): r for r in c[1:]}
    A, B, C = planted
    for strand in '+-':
        assert float(rows[strand, A][head.index('pi_m6A')]) > 0.25 and float(rows[strand, B][head.index('pi_m5C')]) > 0.25
        assert float(rows[strand, C][head.index('pi_can')]) > 0.9
    # without --siteCompose: two files, default names; a refused combination says so
    assert cli.main(argv + ['--FileID', 'plain']) == 0 and not os.path.exists(os.path.join(out, 'plain_site_compose.txt'))
    assert open(os.path.join(out, 'plain_read_llr_multi.txt')).readline().split()[7:9] == ['n_mod_mod1', 'n_mod_mod2']
    assert cli.main(argv + ['--FileID', 'bad', '--fdr', 'bh']) == 1


def test_one_alt_model_writes_the_files_of_before(tmp_path):
    """a single --altModel path takes the code of before K26: the three files have the bytes the parent commit's build wrote"""
    from nanomod_amd import cli
    paths = write_inputs(tmp_path)
    out = str(tmp_path / 'one')
    assert cli.main(single_alt_argv(paths, out)) == 0
    assert sorted(os.listdir(out)) == sorted(PARENT_SHA256)
    got = {name: sha256_of(os.path.join(out, name)) for name in PARENT_SHA256}
    print(got)
    assert got == PARENT_SHA256
