"""nanomod_amd — MI355X (gfx950) implementation of NanoMod's per-base two-sample
testing hot path (KS / Mann-Whitney U / Welch t per genomic position + sliding
window Stouffer / Fisher combine), behind the reference's own Python call
boundary.  See DESIGN.md and INTEGRATION.md."""
from . import _lib  # noqa: F401
from .detect import (mtest2, mfilter_coverage, getKStest, get_combin_pvalue, combin_pvalues,  # noqa: F401
                     pos_check, save_test, m_min_float, m_max_float, run_ids, build_csr, encode_signals, region_rank)
from .engine import detect_host, combine_host, DeviceDetector, EventTimer, fdr_adjust_host, one_sample_host, kmer_model_host, kmer_mix_host, rescale_reads_host, reads_to_group, read_calls_host, site_calls_host, read_llr_host, site_llr_host, site_stoich_host, site_diff_host, match_score_rows, site_diff_rep_host, match_score_rows_multi, pair_index_host, site_pairs_host  # noqa: F401
from .onesample import build_profile, save_profile, load_profile, make_profile, match_positions, mtest1  # noqa: F401
from .kmermodel import (kmer_codes, build_kmer_model, save_kmer_model, load_kmer_model, write_kmer_table,  # noqa: F401
                        model_profile, learn_alt_model, write_kmer_mix_table)
from .rescale import rescale_reads, write_read_scale  # noqa: F401
from .readcalls import call_reads, write_read_calls, write_site_calls  # noqa: F401
from .readllr import call_reads_llr, write_read_llr, write_site_llr, write_site_stoich, compare_reads_llr, write_site_diff, compare_reads_llr_rep, write_site_diff_rep, cooccur_reads_llr, write_site_pairs  # noqa: F401
from .engine import read_llr_multi_host, site_compose_host  # noqa: F401
from .readllr import call_reads_llr_multi, write_read_llr_multi, write_site_llr_multi, write_site_compose  # noqa: F401
from . import simulate, sharding  # noqa: F401

__all__ = ['mtest2', 'mfilter_coverage', 'getKStest', 'get_combin_pvalue', 'combin_pvalues', 'pos_check',
           'save_test', 'm_min_float', 'm_max_float', 'run_ids', 'build_csr', 'encode_signals',
           'detect_host', 'combine_host', 'DeviceDetector', 'EventTimer', 'fdr_adjust_host', 'one_sample_host',
           'build_profile', 'save_profile', 'load_profile', 'make_profile', 'match_positions', 'mtest1',
           'kmer_model_host', 'kmer_codes', 'build_kmer_model', 'save_kmer_model', 'load_kmer_model', 'write_kmer_table', 'model_profile',
           'kmer_mix_host', 'learn_alt_model', 'write_kmer_mix_table',
           'rescale_reads_host', 'reads_to_group', 'rescale_reads', 'write_read_scale',
           'read_calls_host', 'site_calls_host', 'call_reads', 'write_read_calls', 'write_site_calls',
           'read_llr_host', 'site_llr_host', 'call_reads_llr', 'write_read_llr', 'write_site_llr',
           'site_stoich_host', 'write_site_stoich',
           'site_diff_host', 'match_score_rows', 'compare_reads_llr', 'write_site_diff',
           'site_diff_rep_host', 'match_score_rows_multi', 'compare_reads_llr_rep', 'write_site_diff_rep',
           'pair_index_host', 'site_pairs_host', 'cooccur_reads_llr', 'write_site_pairs',
           'read_llr_multi_host', 'site_compose_host', 'call_reads_llr_multi', 'write_read_llr_multi', 'write_site_llr_multi', 'write_site_compose']
