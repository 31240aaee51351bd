"""CPU: tests/pivot_ref.py (the reference the read-pivot step tests compare the device with) against fast5_ingest.GroupBuilder,
and tests/size_steps.py (the mirrored size steps those tests cross) against the kernel sources."""
import os
import re

import numpy as np
import pytest

import pivot_ref as R
import size_steps as Z
from test_read_pivot_gpu import _group_builder, _quiet, _random_reads

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'nanomod_amd', 'csrc')


def _ref_like_cli(reads, opts):
    """the per-read filters, then the event window: what cli does before nmod_pivot_reads"""
    from nanomod_amd import fast5_ingest
    sel = fast5_ingest.select_reads(reads, opts, _quiet)
    lo, hi = (opts['start_pos'], opts['end_pos']) if 'start_pos' in opts and 'end_pos' in opts else (None, None)
    return R.pivot_ref(sel, lo, hi)


@pytest.mark.parametrize('kind', ['f64', 'f32', 'i16'])
def test_pivot_ref_equals_group_builder_on_random_reads(kind):
    rng = np.random.default_rng({'f64': 1, 'f32': 2, 'i16': 3}[kind])
    reads = _random_reads(rng, 900, kind)
    # (the second set is test_pivot_random_reads_equal_group_builder's: no read spans that window, nothing is left)
    for opts, least in (({'min_lr': 0}, 5000), ({'min_lr': 0, 'Chr': 'chr2', 'start_pos': 700, 'end_pos': 1900}, 0),
                        ({'min_lr': 50, 'Chr': 'chr1', 'Pos': 100, 'Pos2': 2500}, 1000),
                        ({'min_lr': 0, 'start_pos': 1000, 'end_pos': 1100}, 300)):
        exp = _group_builder(reads, opts)
        assert len(exp['pos']) >= least, (opts, len(exp['pos']))
        R.same_group(_ref_like_cli(reads, opts), exp)


def _reads(chrom, strand, start, lens, rng, kind='i16'):
    lens = np.asarray(lens, dtype=np.int64)
    off = np.zeros(len(lens) + 1, np.int64); off[1:] = np.cumsum(lens)
    k = rng.integers(-3000, 3000, off[-1])
    vals = {'f64': k / 1000.0 + rng.normal(0, 1e-7, off[-1]), 'f32': (k / 1000.0).astype(np.float32), 'i16': k.astype(np.int16)}[kind]
    return dict(chrom=np.asarray(chrom), strand=np.asarray(strand), start=np.asarray(start, dtype=np.int64), off=off, norm_mean=vals,
                base=rng.choice(np.array(list(b'ACGT'), dtype=np.uint8), off[-1]).view('S1'))


def test_pivot_ref_with_zero_length_reads():
    rng = np.random.default_rng(4)
    # empty reads first, last, next to each other and as a chromosome's only reads ('chrZ' then has no row)
    chrom = ['chrB', 'chrA', 'chrA', 'chrZ', 'chrB', 'chrB', 'chrA', 'chrZ', 'chrA']
    strand = ['+', '-', '+', '+', '-', '-', '-', '-', '+']
    start = [7, 3, 5, 0, 9, 9, 4, 11, 5]
    lens = [0, 4, 3, 0, 0, 5, 2, 0, 0]
    for kind in ('f64', 'i16'):
        reads = _reads(chrom, strand, start, lens, rng, kind)
        exp = _group_builder(reads, {'min_lr': 0})
        assert list(np.unique(exp['chrom'])) == ['chrA', 'chrB'] and exp['off'][-1] == 14
        R.same_group(R.pivot_ref(reads), exp)
    # nothing but empty reads, and no read at all
    R.same_group(R.pivot_ref(_reads(chrom[:2], strand[:2], start[:2], [0, 0], rng)), _group_builder(_reads(chrom[:2], strand[:2], start[:2], [0, 0], rng), {'min_lr': 0}))
    none = _reads(np.zeros(0, str), np.zeros(0, str), [], [], rng)
    got = R.pivot_ref(none)
    assert len(got['pos']) == 0 and list(got['off']) == [0] and len(got['sig']) == 0
    R.same_group(got, _group_builder(none, {'min_lr': 0}))


def test_pivot_ref_one_event_reads_and_reads_clipped_to_nothing(monkeypatch):
    from nanomod_amd import fast5_ingest
    rng = np.random.default_rng(5)
    n = 400
    reads = _reads(rng.choice(np.array(['c1', 'c2']), n), rng.choice(np.array(['+', '-']), n), rng.integers(0, 30, n), np.ones(n, np.int64), rng)
    exp = _group_builder(reads, {'min_lr': 0})
    assert np.diff(exp['off']).max() > 3 and len(exp['pos']) <= 120
    R.same_group(R.pivot_ref(reads), exp)
    # GroupBuilder's own filter keeps a read with start + n == start_pos == end_pos, and the window then leaves nothing of it
    reads = _reads(['c1', 'c1', 'c1'], ['+', '-', '+'], [10, 12, 15], [10, 8, 5], rng)
    opts = {'min_lr': 0, 'start_pos': 20, 'end_pos': 20}
    exp = _group_builder(reads, opts)
    assert list(exp['pos']) == [] and list(exp['off']) == [0]
    R.same_group(_ref_like_cli(reads, opts), exp)
    # the event window on its own (the per-read filters switched off): reads that touch the window with one event, reads it
    # leaves nothing of, on both strands
    monkeypatch.setattr(fast5_ingest, 'read_passes_filters', lambda *a, **k: True)
    chrom = ['c1'] * 8 + ['c2'] * 2
    strand = ['+', '+', '-', '-', '+', '-', '+', '-', '+', '-']
    start = [60, 46, 46, 60, 61, 10, 40, 48, 0, 70]
    lens = [5, 5, 5, 5, 3, 40, 30, 6, 50, 9]
    reads = _reads(chrom, strand, start, lens, rng, 'f64')
    for lo, hi in ((50, 60), (50, 50), (0, 46), (0, 0), (200, 300)):
        exp = _group_builder(reads, {'min_lr': 0, 'start_pos': lo, 'end_pos': hi})
        R.same_group(R.pivot_ref(reads, lo, hi), exp)
    assert len(_group_builder(reads, {'min_lr': 0, 'start_pos': 200, 'end_pos': 300})['pos']) == 0
    assert list(_group_builder(reads, {'min_lr': 0, 'start_pos': 50, 'end_pos': 50})['pos']) == [50, 50]      # one row a strand


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _const(text, name):
    m = re.findall(r'constexpr\s+(?:int|int64_t)\s+(?:\w+\s*=\s*[^,;]+,\s*)*' + name + r'\s*=\s*(\d+)\s*[,;]', text)
    assert len(m) == 1, (name, m)
    return int(m[0])


def test_mirrored_size_steps_equal_the_sources():
    from nanomod_amd import detect
    rs, rp, ro = _src('radix_sort.hpp'), _src('read_pivot.hip'), _src('rank_order.hip')
    rk = _src('radix_sort.hip')                    # the sort's kernels (the header keeps its constants)
    assert _const(rs, 'kRsThreads') == Z.RS_THREADS
    assert _const(rs, 'kRsItems') == Z.RS_ITEMS
    assert _const(rs, 'kRsScanChunk') == Z.RS_SCAN_CHUNK
    assert re.search(r'kRsTile\s*=\s*kRsThreads\s*\*\s*kRsItems\s*;', rs)
    assert _const(rp, 'kScanPer') == Z.SCAN_PER
    assert re.search(r'kScanChunk\s*=\s*256\s*\*\s*kScanPer\s*;', rp)
    assert _const(rp, 'kSmallRow') == Z.SMALL_ROW
    assert _const(rp, 'kWaves') == Z.WAVES
    assert _const(rp, 'kDeviceEncodeAbove') == Z.DEVICE_ENCODE_ABOVE == detect.DEVICE_ENCODE_ABOVE
    assert (1 << _const(rp, 'kPosBits')) == Z.POS_LIMIT
    # the rounds of the two one-block scans are their block size
    assert len(re.findall(r'for \(int64_t b0 = 0; b0 < nb; b0 \+= (\d+)\)', rk)) == 1
    assert int(re.findall(r'for \(int64_t b0 = 0; b0 < nb; b0 \+= (\d+)\)', rk)[0]) == Z.RS_TOPS_ROUND
    assert [int(x) for x in re.findall(r'for \(int64_t b0 = 0; b0 < nb; b0 \+= (\d+)\)', rp)] == [Z.SCAN_TOPS_ROUND]
    # the two grid caps
    assert [int(x) for x in re.findall(r'persistent_grid\(n, per_block, (\d+)\)', rp)] == [Z.PIVOT_GRID_CAP]
    caps = re.findall(r'/ 256 < (\d+) \? \((?:n|cnt) \+ 255\) / 256 : (\d+)\)', ro)
    assert len(caps) == 2 and all(int(a) == int(b) == Z.RANK_GRID_CAP for a, b in caps)
    # what the step tests rely on
    assert Z.RS_ONE_ROUND_MAX == 8388608 and Z.rs_chunk_sums(Z.RS_ONE_ROUND_MAX) == Z.RS_TOPS_ROUND
    assert Z.rs_tiles(Z.RS_ONE_ROUND_MAX + 2049) == 4098 and Z.rs_chunk_sums(Z.RS_ONE_ROUND_MAX + 2049) == Z.RS_TOPS_ROUND + 1
    assert Z.SCAN_ONE_ROUND_MAX == 1048576 and Z.RANK_ONE_SWEEP_MAX == 2097152 and Z.PLACE_ONE_SWEEP_MAX == 262144
