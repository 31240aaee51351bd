"""The moderated replicate comparison (K25) above the engine: the three-call chain that compare_reads_llr_rep(..., moderate=True) runs
in place of nmod_site_diff_rep alone, and the writer of its two files (readllr hands both on under its own name)."""
from __future__ import annotations

import numpy as np

from . import _lib as L
from . import tables as T


def moderated_entry(det, rows, G, n_control, diff):
    """K24 without its interval for phi and status, the prior fitted over them (K25, nmod_rep_prior), K24 again under the prior: three
    calls on one stream, the record never leaves the device in between"""
    first = det.site_diff_rep(rows['sig'], rows['off'], G, n_control, interval=False, **diff)
    prior = det.rep_prior(first['phi'], first['status'], G - 2, ci_level=diff.get('ci_level', 0.95))
    return dict(det.site_diff_rep(rows['sig'], rows['off'], G, n_control, prior=prior, **diff), rep_prior=prior)


def write_site_diff_mod(path, sites, prior_path=None):
    """Two files of compare_reads_llr_rep(..., moderate=True).  <FileID>_site_diff_mod.txt (`path`): write_site_diff_rep's columns up
    to p_rep, the moderated one, then 'phi_post df_tot' as '%.3f %g', then '[q] status'.  <FileID>_rep_prior.txt (prior_path; by
    default beside `path`, its '_site_diff_mod.txt' replaced): one line 'name value' ('%s %.17g') per word of nmod_rep_prior's record,
    in the record's order"""
    G = int(sites['n_samples'])
    nv, ps = np.asarray(sites['n_valid']).reshape(-1, G), np.asarray(sites['pi_s']).reshape(-1, G)
    per = [col.tolist() for g in range(G) for col in (nv[:, g], ps[:, g])]
    q_cols, q_fmt = T.sci_if(sites, 'q')
    T.write_rows(path, '%s %s %d %s %d ' + '%d %.6f ' * G + '%.6f %.6f %.6f %.6f %.6f %.6f %.3f %s %.3f %s %.3f %s %.3f %g ' + q_fmt + '%d\n',
                 T.site_cols(sites, base=True) + [[G] * len(nv)] + per +
                 T.fields(sites, 'pi0', 'pi1', 'pi_pool', 'delta', 'delta_lo', 'delta_hi', 'stat_cond') +
                 [T.sci(sites['p_cond'])] + T.fields(sites, 'stat_het') + [T.sci(sites['p_het'])] + T.fields(sites, 'phi') + [T.sci(sites['p_rep'])] +
                 T.fields(sites, 'phi_post') + [[float(sites['df_tot'])] * len(nv)] + q_cols + T.fields(sites, 'rep_status'))
    if prior_path is None:
        tail = '_site_diff_mod.txt'
        prior_path = (path[:-len(tail)] if path.endswith(tail) else path) + '_rep_prior.txt'
    T.write_rows(prior_path, '%s %.17g\n', [list(L.REP_PRIOR_FIELDS), [sites['rep_prior'][f] for f in L.REP_PRIOR_FIELDS]])
