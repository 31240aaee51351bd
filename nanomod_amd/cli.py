"""`detect`-compatible command line: the reference's `NanoMod.py detect` flags
(NanoMod.py:344-393) over neutral `.npz` containers, array-native end to end: coverage filter and
position intersection (myDetect.py:301-314,421-431) with numpy, the tests + combine on the GPU through
the C ABI, `_sign_test.txt` through nmod_write_sign_test, ranking as myDetect.py:447-462.

    python -m nanomod_amd.cli detect --wrkBase1 groupA.npz --wrkBase2 groupB.npz --FileID run1 --outFolder out/
"""
from __future__ import annotations

import argparse
import ctypes as C
import math
import os
import sys
import time

import numpy as np

from . import _lib as L
from . import container, detect, engine


def build_parser():
    p = argparse.ArgumentParser(prog='nanomod_amd', description='MI355X implementation of NanoMod detect (hot path only)')
    sub = p.add_subparsers(dest='cmd')
    d = sub.add_parser('detect', help='per-base KS / MWU / Welch-t tests + window combine')
    d.add_argument('--outLevel', type=int, default=2, choices=[0, 1, 2, 3])           # NanoMod.py:348
    d.add_argument('--wrkBase1', required=True, help='read group 1: a .npz container (per position or read-level), or a FAST5 folder (needs h5py)')
    d.add_argument('--wrkBase2', required=True, help='read group 2: a .npz container (per position or read-level), or a FAST5 folder (needs h5py)')
    d.add_argument('--min_lr', type=int, default=500)                                  # NanoMod.py:387
    d.add_argument('--min_lr_nb', type=int, default=0)
    d.add_argument('--FileID', default='mod')                                          # NanoMod.py:349
    d.add_argument('--outFolder', default='mRes')                                      # NanoMod.py:350
    d.add_argument('--MinCoverage', type=int, default=5)                               # NanoMod.py:354
    d.add_argument('--topN', type=int, default=30)                                     # NanoMod.py:355
    d.add_argument('--neighborPvalues', type=int, default=2)                           # NanoMod.py:357
    d.add_argument('--WeightsDif', type=float, default=2.0)                            # NanoMod.py:358
    d.add_argument('--testMethod', default='stouffer', choices=['fisher', 'stouffer', 'ks'])   # NanoMod.py:359
    d.add_argument('--rankUse', default='pv', choices=['st', 'pv'])                    # NanoMod.py:361
    d.add_argument('--SaveTest', type=int, default=1, choices=[0, 1])                  # NanoMod.py:362
    d.add_argument('--mstd', type=int, default=0)                                      # NanoMod.py:378
    d.add_argument('--window', type=int, default=21)                                   # NanoMod.py:351
    d.add_argument('--RegionRankbyST', type=int, default=0, choices=[0, 1])            # NanoMod.py:363
    d.add_argument('--percentile', type=float, default=0.1)                            # NanoMod.py:364
    d.add_argument('--WindOvlp', type=int, default=0, choices=[0, 1])                  # NanoMod.py:365
    d.add_argument('--NA', type=str, default='', choices=['', 'A', 'C', 'G', 'T'])     # NanoMod.py:366
    d.add_argument('--Pos', default='', help="region of interest chr:pos[:pos2] (1-based)")        # NanoMod.py:377
    d.add_argument('--plotType', default='Density', choices=['Violin', 'Density'],
                   help='accepted for compatibility: the R plots are outside this build')  # NanoMod.py:385
    d.add_argument('--downsampling_quantile', type=float, default=0.25)                # NanoMod.py:389
    d.add_argument('--downsampling', type=int, default=100)                            # NanoMod.py:390
    d.add_argument('--coverages', type=str, default='0-0')                             # NanoMod.py:392
    d.add_argument('--seed', type=int, default=0, help='seed of the down-sampling draws (the reference is unseeded)')
    d.add_argument('--device', type=int, default=0)
    d.add_argument('--deepCoverage', type=int, default=0, choices=[0, 1],
                   help='1: test positions with a group beyond 65 535 samples (amplicon / plasmid runs) on the deep form '
                   'instead of reporting NaN for them (moptions[\'nmod_deep\'])')
    d.add_argument('--fdr', default='none', choices=['none', 'bh', 'by'],
                   help='bh / by: Benjamini-Hochberg / Benjamini-Yekutieli q-values of the p-value tracks, one family per track over '
                   'all tested positions, written to <FileID>_sign_test_fdr.txt (moptions[\'nmod_fdr\'])')
    d.add_argument('--fdrAlpha', type=float, default=0.05, help='level of the rejected count and p_crit that --fdr reports '
                   '(moptions[\'nmod_fdr_alpha\'])')
    d.add_argument('--mixFraction', default='none', choices=['none', 'equal', 'free'],
                   help='equal / free: the modified fraction of the mixed group per position by a two-component EM (the modified reads '
                   'share the variance of the unmodified ones, or have their own), written to <FileID>_sign_test_mix.txt; with --fdr only '
                   'for the positions it rejects at --fdrAlpha (moptions[\'nmod_mix\']).  The llr column is a score without a p-value')
    d.add_argument('--mixGroup', type=int, default=2, choices=[1, 2],
                   help='which group is the mixture: 1 = --wrkBase1, 2 = --wrkBase2; the other is the unmodified reference '
                   '(moptions[\'nmod_mix_group\'])')
    d.add_argument('--mixMaxIter', type=int, default=200, help='EM iterations at most, 1 .. 10000 (moptions[\'nmod_mix_max_iter\'])')
    d.add_argument('--mixTol', type=float, default=1e-6, help='EM stops when no parameter moved by more than this; 0 = always run '
                   '--mixMaxIter (moptions[\'nmod_mix_tol\'])')
    d.add_argument('--fast5Reader', default='', help="module:function used to read one resquiggled read file, path -> "
                   "(mapped_chrom, mapped_start, mapped_strand, norm_mean[], base[]) | None; default: the h5py reader of "
                   "nanomod_amd.fast5_ingest (Events table + Alignment attributes, myFast5.py:92-126)")
    d.add_argument('--devicePivot', type=int, default=0, choices=[0, 1],
                   help='1: read FAST5 folders as read-level sets and group their events by position on the GPU '
                   '(nmod_pivot_reads), as read-level .npz containers always are')
    pr = sub.add_parser('profile', help='reduce one read group to a per-position control profile (coverage, mean, sd) for detect1')
    pr.add_argument('--outLevel', type=int, default=2, choices=[0, 1, 2, 3])
    pr.add_argument('--wrkBase1', required=True, help='the control read group: a .npz container (per position or read-level)')
    pr.add_argument('--MinCoverage', type=int, default=5)
    pr.add_argument('--outFolder', default='mRes')
    pr.add_argument('--FileID', default='mod', help='the profile is written to <outFolder>/<FileID>_profile.npz')
    pr.add_argument('--device', type=int, default=0)
    o = sub.add_parser('detect1', help='one read group against a stored profile: KS against N(mean, sd^2), t, window combine')
    o.add_argument('--outLevel', type=int, default=2, choices=[0, 1, 2, 3])
    o.add_argument('--wrkBase1', required=True, help='the sample read group: a .npz container (per position or read-level)')
    o.add_argument('--refProfile', required=True, help="a profile written by 'profile' (a control) or by onesample.save_profile (a model)")
    o.add_argument('--FileID', default='mod')
    o.add_argument('--outFolder', default='mRes')
    o.add_argument('--MinCoverage', type=int, default=5)
    o.add_argument('--topN', type=int, default=30)
    o.add_argument('--neighborPvalues', type=int, default=2)
    o.add_argument('--WeightsDif', type=float, default=2.0)
    o.add_argument('--testMethod', default='stouffer', choices=['fisher', 'stouffer', 'ks'])
    o.add_argument('--rankUse', default='pv', choices=['st', 'pv'])
    o.add_argument('--SaveTest', type=int, default=1, choices=[0, 1])
    o.add_argument('--Pos', default='', help="region of interest chr:pos[:pos2] (1-based)")
    o.add_argument('--window', type=int, default=21, help='with --Pos chr:pos: the region is pos +- (window - 1) / 2')
    o.add_argument('--device', type=int, default=0)
    o.add_argument('--fdr', default='none', choices=['none', 'bh', 'by'],
                   help='bh / by: q-values of the t, KS and combined p-value tracks, written to <FileID>_one_sample_fdr.txt')
    o.add_argument('--fdrAlpha', type=float, default=0.05)
    km = sub.add_parser('kmermodel', help='pool a control read group into a k-mer level model (level and spread per k-mer) on the device')
    km.add_argument('--outLevel', type=int, default=2, choices=[0, 1, 2, 3])
    km.add_argument('--wrkBase1', required=True, help='the control read group: a .npz container (per position or read-level)')
    km.add_argument('--kmer', type=int, default=5, help='k, 1 .. 8')
    km.add_argument('--kmerCenter', type=int, default=2, help='offset of the position inside its k-mer in read direction, 0 .. k - 1')
    km.add_argument('--MinCoverage', type=int, default=5)
    km.add_argument('--clipSigma', type=float, default=0.0, help='> 0: re-estimate from the samples within mean +- clipSigma * sd per k-mer')
    km.add_argument('--clipRounds', type=int, default=2, help='clipping passes after the plain one (with --clipSigma > 0)')
    km.add_argument('--outFolder', default='mRes')
    km.add_argument('--FileID', default='mod', help='written: <outFolder>/<FileID>_kmer_model.npz and <FileID>_kmer_model.txt')
    km.add_argument('--device', type=int, default=0)
    kx = sub.add_parser('kmermix', help='learn the modified k-mer model from a mixed (native, partly modified) sample against the k-mer '
                        'model of an unmodified control, on the device: the table --altModel takes, without a fully modified control')
    kx.add_argument('--outLevel', type=int, default=2, choices=[0, 1, 2, 3])
    kx.add_argument('--wrkBase1', required=True, help='the mixed sample: a .npz container (per position or read-level)')
    kx.add_argument('--kmerModel', required=True, help="the unmodified k-mer model, written by 'kmermodel' from the control")
    kx.add_argument('--sites', default='', help="optional: pool only the positions listed in this file, lines 'chrom strand pos' (1-based; "
                    'the first three columns of <FileID>_sign_test.txt, _sign_test_fdr.txt or _site_stoich.txt)')
    kx.add_argument('--MinCoverage', type=int, default=5)
    kx.add_argument('--mixModel', default='free', choices=['equal', 'free'], help="the modified component's variance: the control's, or its own")
    kx.add_argument('--minSamples', type=int, default=1000, help='a k-mer is kept only with at least this many pooled events in its window')
    kx.add_argument('--minPi', type=float, default=0.05, help='... and a modified share of its pooled events of at least this, [0, 1]')
    kx.add_argument('--minShift', type=float, default=1.0, help="... and a modified level at least this many control sd away from the control's")
    kx.add_argument('--maxIter', type=int, default=200, help='EM iterations per k-mer at most, 1 .. 10000')
    kx.add_argument('--tol', type=float, default=1e-6, help='the EM stops when no parameter moved by more than this, >= 0')
    kx.add_argument('--outFolder', default='mRes')
    kx.add_argument('--FileID', default='mod', help='written: <outFolder>/<FileID>_alt_kmer_model.npz and <FileID>_kmer_mix.txt')
    kx.add_argument('--device', type=int, default=0)
    kp = sub.add_parser('kmerprofile',help="the 'model' profile a k-mer model predicts for the positions of a read group, for detect1")
    kp.add_argument('--outLevel', type=int, default=2, choices=[0, 1, 2, 3])
    kp.add_argument('--kmerModel', required=True, help="a k-mer model written by 'kmermodel'")
    kp.add_argument('--wrkBase1', required=True, help='the sample read group: a .npz container (per position or read-level)')
    kp.add_argument('--minPositions', type=int, default=1, help='use a k-mer only if its entry rests on at least this many positions')
    kp.add_argument('--outFolder', default='mRes')
    kp.add_argument('--FileID', default='mod', help='the profile is written to <outFolder>/<FileID>_profile.npz')
    kp.add_argument('--device', type=int, default=0, help='the device that groups a read-level --wrkBase1 by position')
    rs = sub.add_parser('rescale', help='put the reads of a read-level container on the scale of a k-mer model: a per-read shift and '
                        'scale fitted and applied on the device')
    rs.add_argument('--outLevel', type=int, default=2, choices=[0, 1, 2, 3])
    rs.add_argument('--wrkBase1', required=True, help='the sample reads: a read-level .npz container')
    rs.add_argument('--kmerModel', required=True, help="a k-mer model written by 'kmermodel'")
    rs.add_argument('--outReads', required=True, help='the rescaled read-level .npz container to write')
    rs.add_argument('--unweighted', action='store_true', help='fit with equal weights instead of 1 / sd^2 of the k-mer')
    rs.add_argument('--clipSigma', type=float, default=3.0, help='a clipping round keeps the events within clipSigma * scale * sd of the fit')
    rs.add_argument('--clipRounds', type=int, default=2, help='clipping rounds after the plain fit, 0 .. 8')
    rs.add_argument('--minEvents', type=int, default=50, help='a read with fewer fitted events in any round fails')
    rs.add_argument('--scaleLo', type=float, default=0.5, help='a read whose scale lies below fails')
    rs.add_argument('--scaleHi', type=float, default=2.0, help='a read whose scale lies above fails')
    rs.add_argument('--minPositions', type=int, default=1, help='use a k-mer only if its entry rests on at least this many positions')
    rs.add_argument('--dropFailed', action='store_true', help='leave the reads whose fit failed out of --outReads (default: unchanged)')
    rs.add_argument('--outFolder', default='mRes')
    rs.add_argument('--FileID', default='mod', help='the per-read table is written to <outFolder>/<FileID>_read_scale.txt')
    rs.add_argument('--device', type=int, default=0)
    rc = sub.add_parser('readcalls', help='call the events of every read against a k-mer model on the device: which reads are modified '
                        'where, and the share of called reads per position')
    rc.add_argument('--outLevel', type=int, default=2, choices=[0, 1, 2, 3])
    rc.add_argument('--wrkBase1', required=True, help='the sample reads: a read-level .npz container')
    rc.add_argument('--kmerModel', required=True, help="a k-mer model written by 'kmermodel'")
    rc.add_argument('--neighborPvalues', type=int, default=2, help='events of the same read on each side whose p-values are combined '
                    "(Fisher's method), 0 .. 64")
    rc.add_argument('--callAlpha', type=float, default=0.01, help='an event is called when its combined p-value is at most this, (0, 1]')
    rc.add_argument('--minPositions', type=int, default=1, help='use a k-mer only if its entry rests on at least this many positions')
    rc.add_argument('--rescale', type=int, default=0, choices=[0, 1], help="1: put every read on the model's scale first (the fit of "
                    "'rescale' with its defaults, on the device)")
    rc.add_argument('--outEvents', default='', help='optional: a .npz file for the per-event tracks z, p, p_win (with off)')
    rc.add_argument('--outFolder', default='mRes')
    rc.add_argument('--FileID', default='mod', help='written: <outFolder>/<FileID>_read_calls.txt and <FileID>_site_calls.txt')
    rc.add_argument('--device', type=int, default=0)
    rl = sub.add_parser('readllr', help='call the events of every read between an unmodified and a modified k-mer model on the device '
                        '(log-likelihood ratios): modified, canonical or neither, and the modified share per position')
    rl.add_argument('--outLevel', type=int, default=2, choices=[0, 1, 2, 3])
    rl.add_argument('--wrkBase1', required=True, help='the sample reads: a read-level .npz container')
    rl.add_argument('--kmerModel', required=True, help="the unmodified k-mer model, written by 'kmermodel'")
    rl.add_argument('--altModel', required=True, help="the modified k-mer model, written by 'kmermodel' from a fully modified control or learnt by 'kmermix' from a mixed sample"
                    "; or two to four of them, comma-separated: every event is called between canonical and all of these modifications at once "
                    "(<FileID>_read_llr_multi.txt and <FileID>_site_llr_multi.txt)")
    rl.add_argument('--modNames', default='', help='several --altModel: a name per modified model, comma-separated (default mod1,mod2,...)')
    rl.add_argument('--modPrior', default='', help='several --altModel: the prior probability of each modification behind the posterior '
                    'track, comma-separated, their sum below 1 (default: canonical and the modifications alike)')
    rl.add_argument('--siteCompose', type=int, default=0, choices=[0, 1], help='several --altModel, 1: also estimate the shares of all '
                    'modifications at every position by maximum likelihood, with a test per modification (<FileID>_site_compose.txt)')
    rl.add_argument('--composeMaxIter', type=int, default=500, help='--siteCompose: the most EM iterations of a fit, 1 .. %d' % L.COMPOSE_MAX_ITER)
    rl.add_argument('--composeTol', type=float, default=1e-9, help='--siteCompose: a fit stops when no share moves by more than this, >= 0')
    rl.add_argument('--fdr', default='none', choices=['none', 'bh', 'by'], help='--siteCompose: bh / by: q-values of the test of every '
                    'modification over all positions, a column beside each p-value')
    rl.add_argument('--fdrAlpha', type=float, default=0.05)
    rl.add_argument('--llrThreshold', type=float, default=2.5, help='an event is called when its window sum reaches +- this, > 0')
    rl.add_argument('--llrWindow', default='kmer', help="'kmer': the events whose k-mer holds the base; or LO,HI: events of the same read "
                    'before and after, 0 .. 64 each')
    rl.add_argument('--prior', type=float, default=0.5, help='prior probability of the modified state behind p_mod, inside (0, 1)')
    rl.add_argument('--minPositions', type=int, default=1, help='use a k-mer only if its entry rests on at least this many positions')
    rl.add_argument('--rescale', type=int, default=0, choices=[0, 1], help="1: put every read on the unmodified model's scale first (the "
                    "fit of 'rescale' with its defaults, on the device)")
    rl.add_argument('--siteFraction', type=int, default=0, choices=[0, 1], help='1: also estimate the modified share of every position '
                    'by maximum likelihood over all its window sums, with an interval and a test of "nothing is modified" '
                    '(<FileID>_site_stoich.txt)')
    rl.add_argument('--minValid', type=int, default=3, help='--siteFraction: scored reads a position needs for an estimate, > 0')
    rl.add_argument('--ciLevel', type=float, default=0.95, help='--siteFraction: the level of the likelihood interval, inside (0, 1)')
    rl.add_argument('--outEvents', default='', help='optional: a .npz file for the per-event tracks llr, llr_win, p_mod (with off)')
    rl.add_argument('--outFolder', default='mRes')
    rl.add_argument('--FileID', default='mod', help='written: <outFolder>/<FileID>_read_llr.txt and <FileID>_site_llr.txt')
    rl.add_argument('--device', type=int, default=0)
    rd = sub.add_parser('readdiff', help='compare the modified share of every site between two read-level samples on the device: the '
                        'share of each, their difference with a profile-likelihood interval, and the likelihood-ratio test of equal shares')
    rd.add_argument('--outLevel', type=int, default=2, choices=[0, 1, 2, 3])
    rd.add_argument('--wrkBase1', required=True, help='sample 0, the control condition: a read-level .npz container; or its replicates, '
                    'comma-separated (three or more containers in all: the replicate-aware comparison)')
    rd.add_argument('--wrkBase2', required=True, help='sample 1: a read-level .npz container; or its replicates, comma-separated')
    rd.add_argument('--kmerModel', required=True, help="the unmodified k-mer model, written by 'kmermodel'")
    rd.add_argument('--altModel', required=True, help="the modified k-mer model, written by 'kmermodel' from a fully modified control or learnt by 'kmermix' from a mixed sample")
    rd.add_argument('--llrWindow', default='kmer', help="'kmer': the events whose k-mer holds the base; or LO,HI: events of the same read "
                    'before and after, 0 .. 64 each')
    rd.add_argument('--prior', type=float, default=0.5, help='prior probability of the modified state, inside (0, 1)')
    rd.add_argument('--minPositions', type=int, default=1, help='use a k-mer only if its entry rests on at least this many positions')
    rd.add_argument('--rescale', type=int, default=0, choices=[0, 1], help="1: put every read on the unmodified model's scale first")
    rd.add_argument('--minCoverage', type=int, default=1, help='reads a site needs in each sample to be compared, > 0')
    rd.add_argument('--minValid', type=int, default=3, help='scored reads a site needs in each sample for an estimate, > 0')
    rd.add_argument('--ciLevel', type=float, default=0.95, help='the level of the interval of delta, inside (0, 1)')
    rd.add_argument('--phiFloor', type=float, default=0.0, help='replicates only: the dispersion between replicates never counts as less '
                    '(0: as estimated; 1: never below binomial), >= 0')
    rd.add_argument('--moderate', type=int, default=0, choices=[0, 1], help='replicates only (three or more containers): 1: shrink the '
                    'dispersion of every site towards a prior fitted over all sites; p_rep, the interval and --fdr are then the moderated '
                    'ones, written to <FileID>_site_diff_mod.txt and <FileID>_rep_prior.txt')
    rd.add_argument('--fdr', default='none', choices=['none', 'bh', 'by'], help='bh / by: q-values of p_diff (with replicates: of p_rep) over '
                    'all compared sites')
    rd.add_argument('--fdrAlpha', type=float, default=0.05)
    rd.add_argument('--outFolder', default='mRes')
    rd.add_argument('--FileID', default='mod', help='written: <outFolder>/<FileID>_site_diff.txt (with replicates: <FileID>_site_diff_rep.txt)')
    rd.add_argument('--device', type=int, default=0)
    rp = sub.add_parser('readpairs', help='same-read co-occurrence of modification calls at pairs of nearby sites of one read-level sample '
                        'on the device: per pair the 2 x 2 table of the reads called at both sites, log odds ratio, phi and the exact test')
    rp.add_argument('--outLevel', type=int, default=2, choices=[0, 1, 2, 3])
    rp.add_argument('--wrkBase1', required=True, help='the sample reads: a read-level .npz container')
    rp.add_argument('--kmerModel', required=True, help="the unmodified k-mer model, written by 'kmermodel'")
    rp.add_argument('--altModel', required=True, help="the modified k-mer model, written by 'kmermodel' from a fully modified control or learnt by 'kmermix' from a mixed sample")
    rp.add_argument('--sites', default='stoich', help="'stoich': the positions whose modified share (readllr --siteFraction) has a "
                    "Benjamini-Hochberg q of at most --siteAlpha; or a FILE of lines 'chrom strand pos' (1-based; the first three "
                    'columns of <FileID>_site_stoich.txt work)')
    rp.add_argument('--maxDist', type=int, default=100, help='pairs of sites up to this far apart, 1 .. %d' % L.PAIRS_MAX_DIST)
    rp.add_argument('--llrThreshold', type=float, default=2.5, help='a read is called at a site when its window sum reaches +- this, > 0')
    rp.add_argument('--llrWindow', default='kmer', help="'kmer': the events whose k-mer holds the base; or LO,HI: events of the same read "
                    'before and after, 0 .. 64 each')
    rp.add_argument('--prior', type=float, default=0.5, help='prior probability of the modified state, inside (0, 1)')
    rp.add_argument('--minPositions', type=int, default=1, help='use a k-mer only if its entry rests on at least this many positions')
    rp.add_argument('--rescale', type=int, default=0, choices=[0, 1], help="1: put every read on the unmodified model's scale first")
    rp.add_argument('--minReads', type=int, default=10, help='reads called at both sites a pair needs for its statistics, > 0')
    rp.add_argument('--siteAlpha', type=float, default=0.05, help="--sites stoich: the level of the sites' q-values, in (0, 1]")
    rp.add_argument('--fdr', default='none', choices=['none', 'bh', 'by'], help='bh / by: q-values of p_fisher over all pairs')
    rp.add_argument('--fdrAlpha', type=float, default=0.05)
    rp.add_argument('--soft', type=int, default=0, choices=[0, 1], help='1: also the soft linkage of every pair from the window sums of all '
                    'the reads that cover both sites (marginal shares, linkage D with its interval, r, the test of independence), written to '
                    '<FileID>_site_linkage.txt')
    rp.add_argument('--ciLevel', type=float, default=0.95, help='--soft 1: the level of the likelihood interval of D, inside (0, 1)')
    rp.add_argument('--outFolder', default='mRes')
    rp.add_argument('--FileID', default='mod', help='written: <outFolder>/<FileID>_site_pairs.txt')
    rp.add_argument('--device', type=int, default=0)
    rh = sub.add_parser('readhmm', help='per-read two-state HMM smoothing of the window sums at candidate sites of one read-level sample on the '
                        'device: per read and site the posterior of "modified" given the whole read, the modified stretches of every molecule, and '
                        'the log-likelihood with and without correlation along the read')
    rh.add_argument('--outLevel', type=int, default=2, choices=[0, 1, 2, 3])
    rh.add_argument('--wrkBase1', required=True, help='the sample reads: a read-level .npz container')
    rh.add_argument('--kmerModel', '--model', dest='kmerModel', required=True, help="the unmodified k-mer model, written by 'kmermodel'")
    rh.add_argument('--altModel', required=True, help="the modified k-mer model, written by 'kmermodel' from a fully modified control or learnt by 'kmermix' from a mixed sample")
    rh.add_argument('--sites', default='stoich', help="'stoich': the positions whose modified share (readllr --siteFraction) has a "
                    "Benjamini-Hochberg q of at most --siteAlpha; or a FILE of lines 'chrom strand pos' (1-based)")
    rh.add_argument('--hmmPi', type=float, default=None, help='the stationary modified share, 1e-9 .. 1 - 1e-9; default: the mean of the '
                    "candidate sites' estimated shares")
    rh.add_argument('--hmmLength', type=float, default=200.0, help='the correlation length in bases, 1e-3 .. 1e9')
    rh.add_argument('--fitLength', default=None, help='LEN,LEN,...: the length among these with the largest log-likelihood over all reads is used')
    rh.add_argument('--fitHmm', type=int, default=0, choices=[0, 1], help='1: pi and length are fitted by maximum likelihood over all reads, from '
                    '--hmmPi (or its default) and --hmmLength; the trace and the estimates with their intervals are written to <FileID>_hmm_fit.txt; '
                    'not together with --fitLength')
    rh.add_argument('--fixPi', type=int, default=0, choices=[0, 1], help='--fitHmm 1: keep pi and fit the length alone')
    rh.add_argument('--sitePrior', type=int, default=0, choices=[0, 1], help="1: every candidate site gets a prior share of its own, its estimated "
                    'share shrunk towards pi with the weight of --priorReads reads; written to <FileID>_site_prior.txt; with --fitHmm 1 the length '
                    'alone is fitted')
    rh.add_argument('--priorReads', type=float, default=4.0, help='--sitePrior 1: the weight of pi in reads, > 0')
    rh.add_argument('--callPost', type=float, default=0.9, help='the posterior from which an entry is called, inside (0.5, 1)')
    rh.add_argument('--decode', default='posterior', choices=['posterior', 'viterbi', 'both'], help="'posterior': the marginal calls; 'viterbi': "
                    'the most probable path of every read, written to <FileID>_read_viterbi.txt, _read_domains_viterbi.txt and _site_viterbi.txt; '
                    "'both': the two")
    rh.add_argument('--llrThreshold', type=float, default=2.5, help="K13's call threshold (it does not move the window sums), > 0")
    rh.add_argument('--llrWindow', default='kmer', help="'kmer': the events whose k-mer holds the base; or LO,HI: events of the same read "
                    'before and after, 0 .. 64 each')
    rh.add_argument('--prior', type=float, default=0.5, help='prior probability of the modified state, inside (0, 1)')
    rh.add_argument('--minPositions', type=int, default=1, help='use a k-mer only if its entry rests on at least this many positions')
    rh.add_argument('--rescale', type=int, default=0, choices=[0, 1], help="1: put every read on the unmodified model's scale first")
    rh.add_argument('--siteAlpha', type=float, default=0.05, help="--sites stoich: the level of the sites' q-values, in (0, 1]")
    rh.add_argument('--outFolder', default='mRes')
    rh.add_argument('--FileID', default='mod', help='written: <outFolder>/<FileID>_read_hmm.txt, _read_domains.txt and _site_hmm.txt')
    rh.add_argument('--device', type=int, default=0)
    rk = sub.add_parser('readclasses', help='latent-class clustering of the reads of one read-level sample by their modification pattern on the '
                        'device: a mixture of classes of reads, each with a modified share of its own at every candidate site, fitted by EM; per '
                        'read its class and how firmly it belongs to it, per site and class the share')
    rk.add_argument('--outLevel', type=int, default=2, choices=[0, 1, 2, 3])
    rk.add_argument('--wrkBase1', required=True, help='the sample reads: a read-level .npz container')
    rk.add_argument('--kmerModel', '--model', dest='kmerModel', required=True, help="the unmodified k-mer model, written by 'kmermodel'")
    rk.add_argument('--altModel', required=True, help="the modified k-mer model, written by 'kmermodel' from a fully modified control or learnt by 'kmermix' from a mixed sample")
    rk.add_argument('--sites', default='stoich', help="'stoich': the positions whose modified share (readllr --siteFraction) has a "
                    "Benjamini-Hochberg q of at most --siteAlpha; or a FILE of lines 'chrom strand pos' (1-based)")
    rk.add_argument('--classes', default='2', help='C or C,C,...: the number of classes, 1 .. %d; of several the one with the smallest BIC is kept' % L.CLASSES_MAX)
    rk.add_argument('--nInit', type=int, default=4, help='the seeded starts of every number of classes; the best final log-likelihood is kept')
    rk.add_argument('--seed', type=int, default=0, help='the seed of the starts, >= 0')
    rk.add_argument('--maxIter', type=int, default=500, help='the EM steps of a start at most')
    rk.add_argument('--tol', type=float, default=1e-9, help='a start stops when the log-likelihood rises by at most tol * (|ll| + 1)')
    rk.add_argument('--llrThreshold', type=float, default=2.5, help="K13's call threshold (it does not move the window sums), > 0")
    rk.add_argument('--llrWindow', default='kmer', help="'kmer': the events whose k-mer holds the base; or LO,HI: events of the same read "
                    'before and after, 0 .. 64 each')
    rk.add_argument('--prior', type=float, default=0.5, help='prior probability of the modified state, inside (0, 1)')
    rk.add_argument('--minPositions', type=int, default=1, help='use a k-mer only if its entry rests on at least this many positions')
    rk.add_argument('--rescale', type=int, default=0, choices=[0, 1], help="1: put every read on the unmodified model's scale first")
    rk.add_argument('--siteAlpha', type=float, default=0.05, help="--sites stoich: the level of the sites' q-values, in (0, 1]")
    rk.add_argument('--outFolder', default='mRes')
    rk.add_argument('--FileID', default='mod', help='written: <outFolder>/<FileID>_read_classes.txt, _class_sites.txt and _classes_fit.txt')
    rk.add_argument('--device', type=int, default=0)
    return p


def _read_inputs_checked(errs, a, files):
    """the tail the checks of the read-level commands share: the input files exist and --wrkBase1 is a read-level container"""
    for f in files:
        if not os.path.isfile(f):
            errs.append('Error: input %s does not exist' % f)
    if not errs and not container.is_read_level(a.wrkBase1):
        errs.append('Error: --wrkBase1 %s is not a read-level container (per-position containers have no reads)' % a.wrkBase1)
    return errs


def _quiet_log(a, log):
    """the log of a read-level command: `log`, or nothing above --outLevel error"""
    return (lambda *x: None) if a.outLevel > detect.OUTPUT_ERROR else log


def _save(a, say, suffix, write, what, *tables):
    """make --outFolder, write(<outFolder>/<FileID><suffix>, *tables), and with `what` say where it went; returns the path"""
    os.makedirs(a.outFolder, exist_ok=True)
    path = os.path.join(a.outFolder, a.FileID + suffix)
    write(path, *tables)
    if what:
        say('%s saved in %s' % (what, path))
    return path


def parse_classes(text):
    """--classes: the list of counts of 'C' or 'C,C,...'; None for anything else"""
    parts = text.split(',')
    if not parts or not all(q.strip().isdigit() for q in parts):
        return None
    return [int(q) for q in parts]


def validate_readclasses(a):
    """the checks of readclasses, in validate_readhmm's manner"""
    errs = []
    win = parse_llr_window(a.llrWindow)
    if win is None or (win != 'kmer' and not all(0 <= v <= L.MAX_NB for v in win)):
        errs.append("Error: --llrWindow should be 'kmer' or LO,HI with both in 0 .. %d" % L.MAX_NB)
    if not 0.0 < a.llrThreshold < float('inf'):
        errs.append('Error: --llrThreshold should be finite and larger than 0')
    if not 0.0 < a.prior < 1.0:
        errs.append('Error: --prior should lie between 0 and 1, both excluded')
    if a.minPositions < 1:
        errs.append('Error: --minPositions should be larger than 0')
    counts = parse_classes(a.classes)
    if counts is None or not all(1 <= c <= L.CLASSES_MAX for c in counts):
        errs.append('Error: --classes should be C or C,C,... with every C in 1 .. %d' % L.CLASSES_MAX)
    if a.nInit < 1:
        errs.append('Error: --nInit should be larger than 0')
    if a.seed < 0:
        errs.append('Error: --seed should not be negative')
    if a.maxIter < 1:
        errs.append('Error: --maxIter should be larger than 0')
    if not 0.0 <= a.tol < float('inf'):
        errs.append('Error: --tol should be finite and not negative')
    if not 0.0 < a.siteAlpha <= 1.0:
        errs.append('Error: --siteAlpha should be in (0, 1]')
    return _read_inputs_checked(errs, a, (a.wrkBase1, a.kmerModel, a.altModel) + (() if a.sites == 'stoich' else (a.sites,)))


def run_readclasses(a, log=print):
    from . import kmermodel, readllr
    say = _quiet_log(a, log)
    sites = 'stoich' if a.sites == 'stoich' else readllr.read_sites_file(a.sites)
    res = readllr.cluster_reads_llr(container.load_reads(a.wrkBase1), kmermodel.load_kmer_model(a.kmerModel), kmermodel.load_kmer_model(a.altModel),
                                    sites=sites, classes=parse_classes(a.classes), n_init=a.nInit, seed=a.seed, max_iter=a.maxIter, tol=a.tol,
                                    window=parse_llr_window(a.llrWindow), rescale={} if a.rescale else None, site_alpha=a.siteAlpha,
                                    thr=a.llrThreshold, prior=a.prior, min_positions=a.minPositions, device=a.device, log=say)
    _save(a, say, '_read_classes.txt', readllr.write_read_classes, 'Read classes are', res)
    _save(a, say, '_class_sites.txt', readllr.write_class_sites, 'Class shares per site are', res)
    _save(a, say, '_classes_fit.txt', readllr.write_classes_fit, 'The fits are', res)
    return res


def parse_fit_length(text):
    """--fitLength: the list of lengths of 'LEN,LEN,...'; None for anything else"""
    try:
        vals = [float(q) for q in text.split(',')]
    except ValueError:
        return None
    return vals if vals and all(v == v for v in vals) else None


def parse_llr_window(text):
    """--llrWindow: 'kmer', or (lo, hi) of 'LO,HI'; None for anything else"""
    if text == 'kmer':
        return 'kmer'
    parts = text.split(',')
    if len(parts) != 2 or not all(q.strip().isdigit() for q in parts):
        return None
    return int(parts[0]), int(parts[1])


def validate_readllr(a):
    """the checks of readllr"""
    errs = []
    win = parse_llr_window(a.llrWindow)
    if win is None or (win != 'kmer' and not all(0 <= v <= L.MAX_NB for v in win)):
        errs.append("Error: --llrWindow should be 'kmer' or LO,HI with both in 0 .. %d" % L.MAX_NB)
    if not 0.0 < a.llrThreshold < float('inf'):
        errs.append('Error: --llrThreshold should be finite and larger than 0')
    if not 0.0 < a.prior < 1.0:
        errs.append('Error: --prior should lie between 0 and 1, both excluded')
    if a.minPositions < 1:
        errs.append('Error: --minPositions should be larger than 0')
    if a.minValid < 1:
        errs.append('Error: --minValid should be larger than 0')
    if not 0.0 < a.ciLevel < 1.0:
        errs.append('Error: --ciLevel should lie between 0 and 1, both excluded')
    alts = a.altModel.split(',')
    if len(alts) == 1:
        if a.modNames or a.modPrior or a.siteCompose or a.fdr != 'none':
            errs.append('Error: --modNames, --modPrior, --siteCompose and --fdr need several --altModel files, comma-separated')
        return _read_inputs_checked(errs, a, (a.wrkBase1, a.kmerModel, a.altModel))
    if len(alts) > L.MULTI_MAX:
        errs.append('Error: --altModel takes at most %d files' % L.MULTI_MAX)
    if a.siteFraction or a.outEvents:
        errs.append('Error: --siteFraction and --outEvents are for a single --altModel (several: --siteCompose)')
    if a.modNames and len(a.modNames.split(',')) != len(alts):
        errs.append('Error: --modNames should name every --altModel file')
    if a.modPrior and parse_mod_prior(a.modPrior, len(alts)) is None:
        errs.append('Error: --modPrior should hold a probability inside (0, 1) per --altModel file, their sum below 1')
    if not 1 <= a.composeMaxIter <= L.COMPOSE_MAX_ITER:
        errs.append('Error: --composeMaxIter should be in 1 .. %d' % L.COMPOSE_MAX_ITER)
    if not 0.0 <= a.composeTol < float('inf'):
        errs.append('Error: --composeTol should be finite and not negative')
    if a.fdr != 'none' and not a.siteCompose:
        errs.append('Error: --fdr needs --siteCompose 1')
    if not 0.0 < a.fdrAlpha <= 1.0:
        errs.append('Error: --fdrAlpha should be in (0, 1]')
    return _read_inputs_checked(errs, a, (a.wrkBase1, a.kmerModel) + tuple(alts))


def parse_mod_prior(text, n):
    """--modPrior: n probabilities inside (0, 1) whose sum is below 1; None for anything else"""
    try:
        vals = [float(q) for q in text.split(',')]
    except ValueError:
        return None
    return vals if len(vals) == n and all(0.0 < v < 1.0 for v in vals) and sum(vals) < 1.0 else None


def readdiff_samples(a):
    """the containers of readdiff's two conditions: (--wrkBase1's, --wrkBase2's), each a comma-separated list; one file each is the
    two-sample comparison"""
    return a.wrkBase1.split(','), a.wrkBase2.split(',')


def validate_readdiff(a):
    """the checks of readdiff, in validate_readllr's manner"""
    errs = []
    c0, c1 = readdiff_samples(a)
    if len(c0) + len(c1) > L.REP_MAX_SAMPLES:
        errs.append('Error: --wrkBase1 and --wrkBase2 should name at most %d containers in all' % L.REP_MAX_SAMPLES)
    if not (math.isfinite(a.phiFloor) and a.phiFloor >= 0.0):
        errs.append('Error: --phiFloor should be finite and not negative')
    if a.moderate and len(c0) + len(c1) < 3:
        errs.append('Error: --moderate 1 needs replicates: three or more containers in all')
    win = parse_llr_window(a.llrWindow)
    if win is None or (win != 'kmer' and not all(0 <= v <= L.MAX_NB for v in win)):
        errs.append("Error: --llrWindow should be 'kmer' or LO,HI with both in 0 .. %d" % L.MAX_NB)
    if not 0.0 < a.prior < 1.0:
        errs.append('Error: --prior should lie between 0 and 1, both excluded')
    if a.minPositions < 1:
        errs.append('Error: --minPositions should be larger than 0')
    if a.minCoverage < 1:
        errs.append('Error: --minCoverage should be larger than 0')
    if a.minValid < 1:
        errs.append('Error: --minValid should be larger than 0')
    if not 0.0 < a.ciLevel < 1.0:
        errs.append('Error: --ciLevel should lie between 0 and 1, both excluded')
    if not 0.0 < a.fdrAlpha <= 1.0:
        errs.append('Error: --fdrAlpha should be in (0, 1]')
    for f in c0 + c1 + [a.kmerModel, a.altModel]:
        if not os.path.isfile(f):
            errs.append('Error: input %s does not exist' % f)
    if not errs:
        for opt, f in [('--wrkBase1', f) for f in c0] + [('--wrkBase2', f) for f in c1]:
            if not container.is_read_level(f):
                errs.append('Error: %s %s is not a read-level container (per-position containers have no reads)' % (opt, f))
    return errs


def validate_readpairs(a):
    """the checks of readpairs, in validate_readllr's manner"""
    errs = []
    win = parse_llr_window(a.llrWindow)
    if win is None or (win != 'kmer' and not all(0 <= v <= L.MAX_NB for v in win)):
        errs.append("Error: --llrWindow should be 'kmer' or LO,HI with both in 0 .. %d" % L.MAX_NB)
    if not 0.0 < a.llrThreshold < float('inf'):
        errs.append('Error: --llrThreshold should be finite and larger than 0')
    if not 0.0 < a.prior < 1.0:
        errs.append('Error: --prior should lie between 0 and 1, both excluded')
    if a.minPositions < 1:
        errs.append('Error: --minPositions should be larger than 0')
    if not 1 <= a.maxDist <= L.PAIRS_MAX_DIST:
        errs.append('Error: --maxDist should be in 1 .. %d' % L.PAIRS_MAX_DIST)
    if a.minReads < 1:
        errs.append('Error: --minReads should be larger than 0')
    if not 0.0 < a.siteAlpha <= 1.0:
        errs.append('Error: --siteAlpha should be in (0, 1]')
    if not 0.0 < a.fdrAlpha <= 1.0:
        errs.append('Error: --fdrAlpha should be in (0, 1]')
    if not 0.0 < a.ciLevel < 1.0:
        errs.append('Error: --ciLevel should lie between 0 and 1, both excluded')
    return _read_inputs_checked(errs, a, (a.wrkBase1, a.kmerModel, a.altModel) + (() if a.sites == 'stoich' else (a.sites,)))


def validate_readhmm(a):
    """the checks of readhmm, in validate_readpairs' manner"""
    errs = []
    win = parse_llr_window(a.llrWindow)
    if win is None or (win != 'kmer' and not all(0 <= v <= L.MAX_NB for v in win)):
        errs.append("Error: --llrWindow should be 'kmer' or LO,HI with both in 0 .. %d" % L.MAX_NB)
    if not 0.0 < a.llrThreshold < float('inf'):
        errs.append('Error: --llrThreshold should be finite and larger than 0')
    if not 0.0 < a.prior < 1.0:
        errs.append('Error: --prior should lie between 0 and 1, both excluded')
    if a.minPositions < 1:
        errs.append('Error: --minPositions should be larger than 0')
    if a.hmmPi is not None and not 1e-9 <= a.hmmPi <= 1.0 - 1e-9:
        errs.append('Error: --hmmPi should be in 1e-9 .. 1 - 1e-9')
    if not 1e-3 <= a.hmmLength <= 1e9:
        errs.append('Error: --hmmLength should be in 1e-3 .. 1e9')
    if a.fitLength is not None:
        grid = parse_fit_length(a.fitLength)
        if grid is None or not all(1e-3 <= v <= 1e9 for v in grid):
            errs.append('Error: --fitLength should be LEN,LEN,... with every length in 1e-3 .. 1e9')
    if a.fitHmm and a.fitLength is not None:
        errs.append('Error: --fitHmm 1 and --fitLength exclude each other')
    if a.fixPi and not a.fitHmm:
        errs.append('Error: --fixPi 1 needs --fitHmm 1')
    if a.sitePrior and not 0.0 < a.priorReads < float('inf'):
        errs.append('Error: --priorReads should be finite and larger than 0')
    if not 0.5 < a.callPost < 1.0:
        errs.append('Error: --callPost should lie between 0.5 and 1, both excluded')
    if not 0.0 < a.siteAlpha <= 1.0:
        errs.append('Error: --siteAlpha should be in (0, 1]')
    return _read_inputs_checked(errs, a, (a.wrkBase1, a.kmerModel, a.altModel) + (() if a.sites == 'stoich' else (a.sites,)))


def run_readhmm(a, log=print):
    from . import kmermodel, readllr
    say = _quiet_log(a, log)
    sites = 'stoich' if a.sites == 'stoich' else readllr.read_sites_file(a.sites)
    res = readllr.smooth_reads_llr(container.load_reads(a.wrkBase1), kmermodel.load_kmer_model(a.kmerModel), kmermodel.load_kmer_model(a.altModel),
                                   sites=sites, pi=a.hmmPi, length=a.hmmLength, fit_length=None if a.fitLength is None else parse_fit_length(a.fitLength),
                                   call_post=a.callPost, window=parse_llr_window(a.llrWindow), rescale={} if a.rescale else None,
                                   site_alpha=a.siteAlpha, thr=a.llrThreshold, prior=a.prior, min_positions=a.minPositions, device=a.device,
                                   log=say, **({} if a.decode == 'posterior' else {'decode': a.decode}),
                                   **({'fit': 'mle', 'fix_pi': bool(a.fixPi or a.sitePrior)} if a.fitHmm else {}),
                                   **({'site_prior': True, 'prior_reads': a.priorReads} if a.sitePrior else {}))
    files = []
    if a.fitHmm:
        files.append(('_hmm_fit.txt', readllr.write_hmm_fit, 'The fit of pi and length is', res['fit']))
    if a.sitePrior:
        files.append(('_site_prior.txt', readllr.write_site_prior, 'The per-site priors are', res))
    if a.decode != 'viterbi':
        files += [('_read_hmm.txt', readllr.write_read_hmm, 'Read chains are', res), ('_read_domains.txt', readllr.write_read_domains, 'Read domains are', res),
                  ('_site_hmm.txt', readllr.write_site_hmm, 'Smoothed site counts are', res)]
    if a.decode != 'posterior':
        v = res['viterbi']
        files += [('_read_viterbi.txt', readllr.write_read_viterbi, 'Viterbi paths are', v),
                  ('_read_domains_viterbi.txt', readllr.write_read_domains, 'Viterbi domains are', v),
                  ('_site_viterbi.txt', readllr.write_site_viterbi, 'Viterbi site counts are', v)]
    for suffix, write, what, table in files:
        _save(a, say, suffix, write, what, table)
    for v, ll in res['profile']:
        say('length %g: log-likelihood %.6f%s' % (v, ll, ' *' if v == res['length'] else ''))
    return res


def run_readpairs(a, log=print):
    from . import kmermodel, readllr
    say = _quiet_log(a, log)
    sites = 'stoich' if a.sites == 'stoich' else readllr.read_sites_file(a.sites)
    pairs = readllr.cooccur_reads_llr(container.load_reads(a.wrkBase1), kmermodel.load_kmer_model(a.kmerModel),
                                      kmermodel.load_kmer_model(a.altModel), sites=sites, max_dist=a.maxDist, thr=a.llrThreshold,
                                      min_reads=a.minReads, window=parse_llr_window(a.llrWindow), prior=a.prior,
                                      min_positions=a.minPositions, rescale={} if a.rescale else None,
                                      fdr=None if a.fdr == 'none' else a.fdr, fdr_alpha=a.fdrAlpha, site_alpha=a.siteAlpha, device=a.device,
                                      log=say, **(dict(soft=True, ci_level=a.ciLevel) if a.soft else {}))
    _save(a, say, '_site_pairs.txt', readllr.write_site_pairs, 'Site pairs are', pairs)
    if a.soft:
        _save(a, say, '_site_linkage.txt', readllr.write_site_linkage, 'Site linkage is', pairs)
    return pairs


def run_readdiff(a, log=print):
    from . import kmermodel, readllr
    say = _quiet_log(a, log)
    c0, c1 = readdiff_samples(a)
    models = lambda: (kmermodel.load_kmer_model(a.kmerModel), kmermodel.load_kmer_model(a.altModel))
    shared = dict(window=parse_llr_window(a.llrWindow), prior=a.prior, min_positions=a.minPositions, rescale={} if a.rescale else None,
                  min_coverage=a.minCoverage, fdr=None if a.fdr == 'none' else a.fdr, fdr_alpha=a.fdrAlpha, device=a.device, log=say)
    if len(c0) + len(c1) > 2:
        sites = readllr.compare_reads_llr_rep([container.load_reads(f) for f in c0], [container.load_reads(f) for f in c1], *models(),
                                              diff=dict(min_valid=a.minValid, ci_level=a.ciLevel, phi_floor=a.phiFloor), **shared,
                                              **(dict(moderate=True) if a.moderate else {}))
        if a.moderate:
            path = _save(a, say, '_site_diff_mod.txt', readllr.write_site_diff_mod, 'Moderated site comparisons are', sites)
            say('The prior of the dispersions is saved in %s' % (path[:-len('_site_diff_mod.txt')] + '_rep_prior.txt'))
        else:
            _save(a, say, '_site_diff_rep.txt', readllr.write_site_diff_rep, 'Site comparisons are', sites)
    else:
        sites = readllr.compare_reads_llr(container.load_reads(a.wrkBase1), container.load_reads(a.wrkBase2), *models(),
                                          diff=dict(min_valid=a.minValid, ci_level=a.ciLevel), **shared)
        _save(a, say, '_site_diff.txt', readllr.write_site_diff, 'Site comparisons are', sites)
    return sites


def run_readllr(a, log=print):
    from . import kmermodel, readllr
    say = _quiet_log(a, log)
    reads = container.load_reads(a.wrkBase1)
    alts = a.altModel.split(',')
    if len(alts) > 1:                                          # several modifications at once (K26); a single path: what follows, as ever
        res = readllr.call_reads_llr_multi(
            reads, kmermodel.load_kmer_model(a.kmerModel), [kmermodel.load_kmer_model(f) for f in alts],
            names=a.modNames.split(',') if a.modNames else None, priors=parse_mod_prior(a.modPrior, len(alts)) if a.modPrior else None,
            compose=dict(min_valid=a.minValid, max_iter=a.composeMaxIter, tol=a.composeTol) if a.siteCompose else None,
            window=parse_llr_window(a.llrWindow), thr=a.llrThreshold, min_positions=a.minPositions, rescale={} if a.rescale else None,
            fdr=None if a.fdr == 'none' else a.fdr, fdr_alpha=a.fdrAlpha, device=a.device, log=say)
        first = _save(a, say, '_read_llr_multi.txt', readllr.write_read_llr_multi, None, res[0])
        _save(a, say, '_site_llr_multi.txt', readllr.write_site_llr_multi, None, res[1])
        if a.siteCompose:
            _save(a, say, '_site_compose.txt', readllr.write_site_compose, None, res[1])
        say('Read calls are saved in %s' % first)
        return res
    res = readllr.call_reads_llr(reads, kmermodel.load_kmer_model(a.kmerModel), kmermodel.load_kmer_model(a.altModel),
                                 window=parse_llr_window(a.llrWindow), thr=a.llrThreshold, prior=a.prior, min_positions=a.minPositions,
                                 rescale={} if a.rescale else None, events=bool(a.outEvents), device=a.device, log=say,
                                 **(dict(stoich=dict(min_valid=a.minValid, ci_level=a.ciLevel)) if a.siteFraction else {}))
    table, sites = res[0], res[1]
    first = _save(a, say, '_read_llr.txt', readllr.write_read_llr, None, table)
    _save(a, say, '_site_llr.txt', readllr.write_site_llr, None, sites)
    if a.siteFraction:
        _save(a, say, '_site_stoich.txt', readllr.write_site_stoich, None, sites)
    if a.outEvents:
        np.savez(a.outEvents, off=np.asarray(reads['off'], dtype=np.int64), **res[2])
    say('Read calls are saved in %s' % first)                  # (the first file alone is announced)
    return res


def validate_readcalls(a):
    """the checks of readcalls"""
    errs = []
    if not 0 <= a.neighborPvalues <= L.MAX_NB:
        errs.append('Error: --neighborPvalues should be in 0 .. %d' % L.MAX_NB)
    if not 0.0 < a.callAlpha <= 1.0:
        errs.append('Error: --callAlpha should be larger than 0 and not larger than 1')
    if a.minPositions < 1:
        errs.append('Error: --minPositions should be larger than 0')
    return _read_inputs_checked(errs, a, (a.wrkBase1, a.kmerModel))


def run_readcalls(a, log=print):
    from . import kmermodel, readcalls
    say = _quiet_log(a, log)
    reads = container.load_reads(a.wrkBase1)
    res = readcalls.call_reads(reads, kmermodel.load_kmer_model(a.kmerModel), nb=a.neighborPvalues, alpha=a.callAlpha,
                               min_positions=a.minPositions, rescale={} if a.rescale else None, events=bool(a.outEvents), device=a.device, log=say)
    table, sites = res[0], res[1]
    first = _save(a, say, '_read_calls.txt', readcalls.write_read_calls, None, table)
    _save(a, say, '_site_calls.txt', readcalls.write_site_calls, None, sites)
    if a.outEvents:
        np.savez(a.outEvents, off=np.asarray(reads['off'], dtype=np.int64), **res[2])
    say('Read calls are saved in %s' % first)                  # (the first file alone is announced)
    return res


def validate_rescale(a):
    """the checks of rescale"""
    errs = []
    if not 0 <= a.clipRounds <= 8:
        errs.append('Error: --clipRounds should be in 0 .. 8')
    if a.clipRounds > 0 and not 0.0 < a.clipSigma < float('inf'):
        errs.append('Error: --clipSigma should be finite and positive')
    if a.minEvents < 2:
        errs.append('Error: --minEvents should be not less than 2')
    if not (0.0 < a.scaleLo < float('inf') and a.scaleLo <= a.scaleHi):
        errs.append('Error: --scaleLo should be positive, finite and not above --scaleHi')
    if a.minPositions < 1:
        errs.append('Error: --minPositions should be larger than 0')
    return _read_inputs_checked(errs, a, (a.wrkBase1, a.kmerModel))


def run_rescale(a, log=print):
    from . import kmermodel, rescale
    say = _quiet_log(a, log)
    reads = container.load_reads(a.wrkBase1)
    out, table = rescale.rescale_reads(reads, kmermodel.load_kmer_model(a.kmerModel), weighted=not a.unweighted, clip_sigma=a.clipSigma,
                                       clip_rounds=a.clipRounds, min_events=a.minEvents, scale_range=(a.scaleLo, a.scaleHi),
                                       min_positions=a.minPositions, drop_failed=a.dropFailed, device=a.device, log=say)
    container.save_reads(a.outReads, out['chrom'], out['strand'], out['start'], out['off'], out['norm_mean'], out['base'])
    _save(a, say, '_read_scale.txt', rescale.write_read_scale, None, reads, table)
    say('Rescaled reads are saved in %s' % a.outReads)
    return out, table


def load_group_input(path, device=0):
    """a per-position container; a read-level one is grouped by position on the device first (engine.reads_to_group)"""
    if container.is_read_level(path):
        return engine.reads_to_group(container.load_reads(path), device)
    return container.load_group(path)


def validate_kmer(a):
    """the checks of kmermodel / kmerprofile"""
    errs = []
    inputs = [a.wrkBase1]
    if a.cmd == 'kmermodel':
        if a.MinCoverage < 3:
            errs.append('Error: --MinCoverage should be not less than 3')
        if not 1 <= a.kmer <= 8:
            errs.append('Error: --kmer should be in 1 .. 8')
        elif not 0 <= a.kmerCenter < a.kmer:
            errs.append('Error: --kmerCenter should be in 0 .. kmer - 1')
        if not 0.0 <= a.clipSigma < float('inf'):
            errs.append('Error: --clipSigma should be finite and not negative')
        if a.clipRounds < 0:
            errs.append('Error: --clipRounds should not be negative')
    else:
        inputs.append(a.kmerModel)
        if a.minPositions < 1:
            errs.append('Error: --minPositions should be larger than 0')
    for f in inputs:
        if not os.path.isfile(f):
            errs.append('Error: input %s does not exist' % f)
    return errs


def run_kmermodel(a, log=print):
    from . import kmermodel
    quiet = a.outLevel > detect.OUTPUT_ERROR
    model = kmermodel.build_kmer_model(load_group_input(a.wrkBase1, a.device), a.kmer, a.kmerCenter, a.MinCoverage, a.clipSigma, a.clipRounds,
                                       a.device, (lambda *x: None) if quiet else log)
    os.makedirs(a.outFolder, exist_ok=True)
    path = os.path.join(a.outFolder, a.FileID + '_kmer_model.npz')
    kmermodel.save_kmer_model(path, model)
    kmermodel.write_kmer_table(os.path.join(a.outFolder, a.FileID + '_kmer_model.txt'), model)
    if not quiet:
        log('K-mer model is saved in %s' % path)
    return model


def validate_kmermix(a):
    """the checks of kmermix"""
    errs = []
    if a.MinCoverage < 3:
        errs.append('Error: --MinCoverage should be not less than 3')
    if a.minSamples < 2:
        errs.append('Error: --minSamples should be not less than 2')
    if not 0.0 <= a.minPi <= 1.0:
        errs.append('Error: --minPi should be in [0, 1]')
    if not 0.0 <= a.minShift < float('inf'):
        errs.append('Error: --minShift should be finite and not negative')
    if not 1 <= a.maxIter <= 10000:
        errs.append('Error: --maxIter should be in 1 .. 10000')
    if not 0.0 <= a.tol < float('inf'):
        errs.append('Error: --tol should be finite and not negative')
    for f in (a.wrkBase1, a.kmerModel) + ((a.sites,) if a.sites else ()):
        if not os.path.isfile(f):
            errs.append('Error: input %s does not exist' % f)
    return errs


def run_kmermix(a, log=print):
    from . import kmermodel, readllr
    quiet = a.outLevel > detect.OUTPUT_ERROR
    model = kmermodel.load_kmer_model(a.kmerModel)
    alt, table = kmermodel.learn_alt_model(load_group_input(a.wrkBase1, a.device), model, readllr.read_sites_file(a.sites) if a.sites else None,
                                           a.MinCoverage, a.mixModel, a.maxIter, a.tol, a.minSamples, a.minPi, a.minShift, a.device,
                                           (lambda *x: None) if quiet else log)
    os.makedirs(a.outFolder, exist_ok=True)
    path = os.path.join(a.outFolder, a.FileID + '_alt_kmer_model.npz')
    kmermodel.save_kmer_model(path, alt)
    kmermodel.write_kmer_mix_table(os.path.join(a.outFolder, a.FileID + '_kmer_mix.txt'), model, table)
    if not quiet:
        log('Modified k-mer model is saved in %s' % path)
    return alt, table


def run_kmerprofile(a, log=print):
    from . import kmermodel, onesample
    prof = kmermodel.model_profile(kmermodel.load_kmer_model(a.kmerModel), load_group_input(a.wrkBase1, a.device), a.minPositions)
    os.makedirs(a.outFolder, exist_ok=True)
    path = os.path.join(a.outFolder, a.FileID + '_profile.npz')
    onesample.save_profile(path, prof)
    if a.outLevel <= detect.OUTPUT_ERROR:
        log('Profile of %d positions is saved in %s' % (len(prof['pos']), path))
    return prof


def validate1(a):
    """the checks of validate() that concern profile / detect1"""
    errs = []
    if a.MinCoverage < 3:
        errs.append('Error: --MinCoverage should be not less than 3')
    inputs = [a.wrkBase1]
    if a.cmd == 'detect1':
        inputs.append(a.refProfile)
        if a.topN < 1:
            errs.append('Error: --topN should be larger than 0')
        if not 0 <= a.neighborPvalues <= L.MAX_NB:
            errs.append('Error: --neighborPvalues should be in 0 .. %d' % L.MAX_NB)
        if a.WeightsDif < 1.0:
            a.WeightsDif = 1.0
        if not 0.0 < a.fdrAlpha <= 1.0:
            errs.append('Error: --fdrAlpha should be in (0, 1]')
        a.wrkBase2, a.mixMaxIter, a.mixTol, a.percentile = a.wrkBase1, 200, 1e-6, 0.1           # (validate() reads them)
        errs += [e for e in validate(a) if e not in errs]
    for f in inputs:
        if not os.path.isfile(f):
            errs.append('Error: input %s does not exist' % f)
    return errs


def run_profile(a, log=print):
    from . import onesample
    prof = onesample.build_profile(load_group_input(a.wrkBase1, a.device), a.MinCoverage, a.device, log)
    os.makedirs(a.outFolder, exist_ok=True)
    path = os.path.join(a.outFolder, a.FileID + '_profile.npz')
    onesample.save_profile(path, prof)
    if a.outLevel <= detect.OUTPUT_ERROR:
        log('Profile of %d positions is saved in %s' % (len(prof['pos']), path))
    return prof


def run_detect1(a, log=print):
    from . import onesample
    mo = {'ds2': ['sample'], 'sample': {'nmod_container': load_input(a.wrkBase1, a, log)}, 'nmod_profile': a.refProfile,
          'MinCoverage': a.MinCoverage, 'neighborPvalues': a.neighborPvalues, 'WeightsDif': a.WeightsDif, 'testMethod': a.testMethod,
          'rankUse': a.rankUse, 'SaveTest': a.SaveTest, 'outFolder': a.outFolder, 'FileID': a.FileID, 'outLevel': a.outLevel,
          'nmod_device': a.device, 'nmod_fdr': '' if a.fdr == 'none' else a.fdr, 'nmod_fdr_alpha': a.fdrAlpha}
    order = onesample.mtest1(mo)
    if a.fdr != 'none' and a.outLevel <= detect.OUTPUT_INFO:
        for name, s in mo['nmod_fdr_summary'].items():
            log('FDR %s %s alpha=%g: tested %d excluded %d rejected %d p_crit %.3E'
                % (a.fdr, name, a.fdrAlpha, s['tested'], s['excluded'], s['rejected'], s['p_crit']))
    return mo['one_sample_meta'], mo['one_sample_arrays'], order


def validate(a):
    """NanoMod.py:40-97 (mCommonParam): the checks that concern this path."""
    errs = []
    if a.MinCoverage < 3:
        errs.append('Error: --MinCoverage should be not less than 3')                 # NanoMod.py:65-67
    if a.topN < 1:
        errs.append('Error: --topN should be larger than 0')
    if a.neighborPvalues < 0:
        errs.append('Error: --neighborPvalues should not be negative')
    if a.neighborPvalues > L.MAX_NB:
        errs.append('Error: --neighborPvalues larger than %d is not supported' % L.MAX_NB)
    if a.WeightsDif < 1.0:                                                             # NanoMod.py:76-78: floor at 1.0
        a.WeightsDif = 1.0
    if (a.window - 1) // 2 < 1:                                                        # NanoMod.py:51-53
        errs.append('Window size (%d) is too small' % a.window)
    a.percentile = 0.0 if a.percentile < 0 else (0.99 if a.percentile >= 1 else a.percentile)   # NanoMod.py:91-92
    a.roi = {}                                                                         # NanoMod.py:117-129
    if a.Pos != '':
        mpos = a.Pos.split(':')
        a.roi['Chr'] = mpos[0]
        if len(mpos) > 1:
            a.roi['Pos'] = int(mpos[1]) - 1
            if a.roi['Pos'] < 0:
                errs.append('The position (%d) of interest should not be less than 0' % a.roi['Pos'])
        if len(mpos) > 2:
            a.roi['Pos2'] = int(mpos[2]) - 1
            if a.roi['Pos2'] < 0:
                errs.append('The position (%d) of interest should not be less than 0' % a.roi['Pos2'])
            if a.roi['Pos2'] - a.roi['Pos'] < 1:
                errs.append('The end position (%d) is not larger than the start position (%d)' % (a.roi['Pos2'], a.roi['Pos']))
        if 'Pos' in a.roi and 'Pos2' not in a.roi:                                     # myDetect.py:550-558
            neighbors = (a.window - 1) // 2
            a.roi['start_pos'] = max(a.roi['Pos'] - neighbors, 0)
            a.roi['end_pos'] = a.roi['Pos'] + neighbors
    if not 1 <= getattr(a, 'mixMaxIter', 200) <= 10000:
        errs.append('Error: --mixMaxIter should be in 1 .. 10000')
    if not 0.0 <= getattr(a, 'mixTol', 1e-6) < float('inf'):
        errs.append('Error: --mixTol should be finite and not negative')
    for f in (a.wrkBase1, a.wrkBase2):
        if not (os.path.isfile(f) or os.path.isdir(f)):
            errs.append('Error: input %s does not exist' % f)
    return errs


def _chrom_codes(*chrom_arrays):
    """sorted chromosome names over all inputs and, per input, the index of every entry's name.  Chromosome columns are
    long runs of one name: only the first entry of every run is looked up (np.unique over 9 M strings was half of
    select_positions)."""
    runs = []
    for c in chrom_arrays:
        c = np.asarray(c)
        if len(c) == 0:
            runs.append((c[:0], np.zeros(0, np.int64)))
            continue
        heads = np.flatnonzero(np.r_[True, c[1:] != c[:-1]])
        runs.append((c[heads], np.diff(np.r_[heads, len(c)])))
    heads_all = np.concatenate([r[0] for r in runs]) if runs else np.zeros(0, dtype=str)
    names = np.unique(heads_all)
    out = [np.repeat(np.searchsorted(names, vals), lens).astype(np.int64) for vals, lens in runs]
    return [str(n) for n in names.tolist()], out


def _keys(g, cid):
    sid = (g['strand'] == '-').astype(np.int64)                                       # '+' sorts before '-'
    return (cid << 41) | (sid << 40) | g['pos'].astype(np.int64)


def select_positions(g0, g1, min_coverage, out_level=detect.OUTPUT_ERROR, log=print):
    """Coverage filter + intersection + ordering: the tested-position set of mtest2 as CSR arrays."""
    # mfilter_coverage (myDetect.py:301-314): per group
    keep0 = np.nonzero(np.diff(g0['off']) >= min_coverage)[0]
    keep1 = np.nonzero(np.diff(g1['off']) >= min_coverage)[0]
    names, (cid0, cid1) = _chrom_codes(g0['chrom'], g1['chrom'])
    k0, k1 = _keys(g0, cid0)[keep0], _keys(g1, cid1)[keep1]
    # positions present in both groups, in sorted (chrom, strand, pos) order (myDetect.py:421,427-431)
    if len(k0) == len(k1) and (len(k0) < 2 or bool(np.all(k0[1:] > k0[:-1]))) and np.array_equal(k0, k1):
        common, rows0, rows1 = k0, keep0, keep1          # the same sorted positions in both groups: nothing to intersect
    else:
        common, i0, i1 = np.intersect1d(k0, k1, assume_unique=True, return_indices=True)
        rows0, rows1 = keep0[i0], keep1[i1]
    sig0, off0 = container.gather_rows(g0['sig'], g0['off'], rows0)
    sig1, off1 = container.gather_rows(g1['sig'], g1['off'], rows1)
    npos = len(common)
    chrom = g1['chrom'][rows1]; strand = g1['strand'][rows1]; pos = g1['pos'][rows1]; base = g1['base'][rows1]
    mism = np.nonzero(g0['base'][rows0] != base)[0]
    if out_level <= detect.OUTPUT_ERROR:
        for i in mism[:20]:
            log('Error not equal', (chrom[i], strand[i]), int(pos[i]), base[i], g0['base'][rows0][i])
    if npos:
        sig0, sig1 = detect.encode_pair(np.asarray(sig0), np.asarray(sig1))
    else:
        sig0 = sig1 = np.zeros(0, np.float32)
    rid = detect.run_ids(chrom, strand, pos)
    n0 = np.diff(off0).astype(np.int32); n1 = np.diff(off1).astype(np.int32)
    meta = dict(chrom=chrom, strand=strand, pos=pos, base=base, n0=n0, n1=n1, names=names,
                chrom_id=cid1[rows1].astype(np.int32))
    return meta, sig0, off0, sig1, off1, rid


def load_input(path, a, log=print):
    """A `.npz` container, or a folder of resquiggled FAST5 files read like ReadAllFast5 (myDetect.py:547-633)."""
    if os.path.isdir(path):
        from . import fast5_ingest
        opts = {'min_lr': a.min_lr, 'min_lr_nb': a.min_lr_nb}
        opts.update(getattr(a, 'roi', {}))                                              # read- and event-level filters
        reader = None
        if getattr(a, 'fast5Reader', ''):
            import importlib
            mod, _, fn = a.fast5Reader.partition(':')
            reader = getattr(importlib.import_module(mod), fn)
        return fast5_ingest.ingest_folder(path, opts, reader=reader, log=log)
    g = load_group_input(path, getattr(a, 'device', 0))
    roi = getattr(a, 'roi', {})
    if roi:
        # a container holds aggregated positions: only the position-level part of the region filter applies
        # (myDetect.py:72,112-114); the read-level parts need the reads (FAST5 folders)
        keep = g['chrom'] == roi['Chr']
        if 'start_pos' in roi:
            keep &= (g['pos'] >= roi['start_pos']) & (g['pos'] <= roi['end_pos'])
        rows = np.flatnonzero(keep)
        sig, off = container.gather_rows(g['sig'], g['off'], rows)
        g = dict(chrom=g['chrom'][rows], strand=g['strand'][rows], pos=g['pos'][rows], base=g['base'][rows], off=off, sig=sig)
    return g


def _read_filters(a):
    opts = {'min_lr': a.min_lr, 'min_lr_nb': a.min_lr_nb}
    opts.update(getattr(a, 'roi', {}))
    return opts


def _fast5_reader(a):
    if not getattr(a, 'fast5Reader', ''):
        return None
    import importlib
    mod, _, fn = a.fast5Reader.partition(':')
    return getattr(importlib.import_module(mod), fn)


def is_read_level_input(path, a):
    """read-level .npz containers, and FAST5 folders under --devicePivot 1, take the device route"""
    return container.is_read_level(path) or (os.path.isdir(path) and bool(getattr(a, 'devicePivot', 0)))


def load_reads(path, a, log=print):
    """a read-level input as a filtered read set (the per-read filters of myDetect.py:76-103; the event-level window is the
    pivot's)"""
    from . import fast5_ingest
    if os.path.isdir(path):
        return fast5_ingest.ingest_folder_reads(path, _read_filters(a), reader=_fast5_reader(a), log=log)
    return fast5_ingest.select_reads(container.load_reads(path), _read_filters(a), log)


def select_positions_device(a, log=print):
    """The device route: read-level groups pivoted on the GPU (a per-position container beside one is uploaded as it is), then
    the coverage filter, intersection and gather of the tested rows there.  Returns select_positions' tuple with the CSR
    arrays and run ids as device tensors."""
    roi = getattr(a, 'roi', {})
    pos_lo, pos_hi = (roi['start_pos'], roi['end_pos']) if 'start_pos' in roi and 'end_pos' in roi else (None, None)
    inputs = []
    for path in (a.wrkBase1, a.wrkBase2):
        inputs.append(('reads', load_reads(path, a, log)) if is_read_level_input(path, a) else ('group', load_input(path, a, log)))
    names = sorted(set(engine.chrom_names(*[x for kind, x in inputs if kind == 'reads'])) |
                   set(str(c) for kind, x in inputs if kind == 'group' for c in np.unique(np.asarray(x['chrom']).astype(str)).tolist()))
    groups = [engine.pivot_reads(x, a.device, pos_lo, pos_hi, names=names) if kind == 'reads' else engine.group_to_device(x, names, a.device)
              for kind, x in inputs]
    return engine.select_tested(groups[0], groups[1], a.MinCoverage, a.device, a.outLevel, log)


def nmod_options(a):
    """The moptions keys of this build (detect.mtest2) that the command line sets."""
    return {'nmod_device': a.device, 'nmod_seed': a.seed, 'nmod_deep': int(a.deepCoverage),
            'nmod_fdr': '' if getattr(a, 'fdr', 'none') == 'none' else a.fdr, 'nmod_fdr_alpha': float(getattr(a, 'fdrAlpha', 0.05)),
            'nmod_mix': '' if getattr(a, 'mixFraction', 'none') == 'none' else a.mixFraction, 'nmod_mix_group': int(getattr(a, 'mixGroup', 2)),
            'nmod_mix_max_iter': int(getattr(a, 'mixMaxIter', 200)), 'nmod_mix_tol': float(getattr(a, 'mixTol', 1e-6))}


def run_detect(a, log=print):
    deep = bool(nmod_options(a)['nmod_deep'])
    engine.warm_up(a.device)                                    # HIP start-up beside the loading of the inputs
    method, nb = a.testMethod, a.neighborPvalues
    dev_method = method if (method in ('stouffer', 'fisher') and nb > 0) else 'ks'
    if is_read_level_input(a.wrkBase1, a) or is_read_level_input(a.wrkBase2, a):
        # read-level groups: grouped, filtered and gathered on the GPU; the tests run on the device-resident rows
        t0 = time.time()
        meta, sig0, off0, sig1, off1, rid = select_positions_device(a, log)
        npos = len(meta['pos'])
        if npos:
            det = engine.DeviceDetector(a.device, nb=nb, weights_dif=a.WeightsDif, method=dev_method, want_mstd=a.mstd != 0, deep=deep)
            res = {k: v.cpu().numpy() for k, v in det.run(sig0, sig1, rid, off0=off0, off1=off1).items()}
        else:
            e = np.zeros(0, np.float32)
            res = engine.detect_host(e, np.zeros(1, np.int64), e, np.zeros(1, np.int64), np.zeros(0, np.int32), nb=nb,
                                     weights_dif=a.WeightsDif, method=dev_method, want_mstd=a.mstd != 0, device=a.device, deep=deep)
        cov = [int(x) for x in a.coverages.split('-')]
        if npos and any(c > 0 for c in cov):           # the down-sampling step reads host arrays
            sig0, off0, sig1, off1, rid = (x.cpu().numpy() for x in (sig0, off0, sig1, off1, rid))
    else:
        g0, g1 = load_input(a.wrkBase1, a, log), load_input(a.wrkBase2, a, log)
        t0 = time.time()
        meta, sig0, off0, sig1, off1, rid = select_positions(g0, g1, a.MinCoverage, a.outLevel, log)
        npos = len(rid)
        res = engine.detect_host(sig0, off0, sig1, off1, rid, nb=nb, weights_dif=a.WeightsDif, method=dev_method,
                                 want_mstd=a.mstd != 0, device=a.device, deep=deep)
    chrom, strand, pos, base = meta['chrom'], meta['strand'], meta['pos'], meta['base']
    if npos and np.any(res['status'] & L.STATUS_MWU_ALL_IDENTICAL):
        raise ValueError('All numbers are identical in mannwhitneyu')                  # scipy 1.2.1, uncaught in the reference
    cov = [int(x) for x in a.coverages.split('-')]                                     # NanoMod.py:174-176
    if npos:
        detect.downsample_update(res, sig0, off0, sig1, off1, rid, strand, cov * 2 if len(cov) == 1 else cov,
                                 iters=a.downsampling, quantile=a.downsampling_quantile, seed=a.seed, nb=nb,
                                 weights_dif=a.WeightsDif, method=dev_method, device=a.device, deep=deep)
    if a.outLevel <= detect.OUTPUT_INFO:
        log('Producing pvalues: consuming time %d' % (time.time() - t0))
    if method != 'ks' and nb == 0:                                                     # myDetect.py:413
        res['comb_st'], res['comb_p'] = res['ks_d'].copy(), res['ks_p'].copy()
    os.makedirs(a.outFolder, exist_ok=True)
    opts = nmod_options(a)
    fdr = None
    if opts['nmod_fdr']:                                                               # q-values of the table's p-value tracks
        fdr, fdr_summary = detect.fdr_tracks(res, method != 'ks' and nb >= 0, opts['nmod_fdr'], opts['nmod_fdr_alpha'], a.device)
        if a.outLevel <= detect.OUTPUT_INFO:
            for name, s in fdr_summary.items():
                log('FDR %s %s alpha=%g: tested %d excluded %d rejected %d p_crit %.3E'
                    % (opts['nmod_fdr'], name, opts['nmod_fdr_alpha'], s['tested'], s['excluded'], s['rejected'], s['p_crit']))
    mix = None
    if opts['nmod_mix']:                                                               # modified fraction per (rejected) position
        if not isinstance(sig0, np.ndarray):                                  # (the device route's tensors: this step reads host rows)
            sig0, off0, sig1, off1 = (x.cpu().numpy() for x in (sig0, off0, sig1, off1))
        gate = None if fdr is None else fdr['comb_q' if (method != 'ks' and nb >= 0) else 'ks_q']
        mix = detect.mix_tracks(sig0, off0, sig1, off1, opts['nmod_mix'], group=opts['nmod_mix_group'], max_iter=opts['nmod_mix_max_iter'],
                                tol=opts['nmod_mix_tol'], gate=gate, gate_max=opts['nmod_fdr_alpha'], device=a.device)
        if a.outLevel <= detect.OUTPUT_INFO:
            done = ~((mix['status'] & L.MIX_SKIPPED) != 0)
            log('MIX %s group %d: computed %d of %d positions, not converged %d, degenerate %d'
                % (opts['nmod_mix'], opts['nmod_mix_group'], int(done.sum()), npos, int(((mix['status'] & L.MIX_NOT_CONVERGED) != 0).sum()),
                   int(((mix['status'] & L.MIX_DEGENERATE) != 0).sum())))
    if a.SaveTest:
        with_comb = nb > 0 and method != 'ks'                                          # myDetect.py:533
        path = os.path.join(a.outFolder, a.FileID + '_sign_test.txt')
        write_sign_test(path, meta, res, with_comb)
        if fdr is not None:
            detect.write_sign_test_fdr(os.path.join(a.outFolder, a.FileID + '_sign_test_fdr.txt'), meta, fdr)
        if mix is not None:
            detect.write_sign_test_mix(os.path.join(a.outFolder, a.FileID + '_sign_test_mix.txt'), meta, mix)
        if a.outLevel <= detect.OUTPUT_ERROR:
            log('Test data is saved in', path)
        if a.mstd != 0:
            with open(os.path.join(a.outFolder, a.FileID + '_meanstd.cvs'), 'w') as mw:   # myDetect.py:541-544
                for i in range(npos):
                    mw.write('%s %s %d %s %.3f %.3f %.3f %.3f\n' % (chrom[i], strand[i], pos[i], base[i], res['mean0'][i],
                                                                    res['std0'][i], res['mean1'][i], res['std1'][i]))
    if a.RegionRankbyST == 0:
        order = rank_order(res, method, a.rankUse, a.device)
    else:                                                                              # myDetect.py:463-515
        recs = []
        for i in range(npos):
            t = [(res['mwu_u'][i], res['mwu_p'][i]), (res['t_t'][i], res['t_p'][i]), (res['ks_d'][i], res['ks_p'][i])]
            if method != 'ks':
                t.append((res['comb_st'][i], res['comb_p'][i]))
            recs.append(((str(chrom[i]), str(strand[i]), int(pos[i]), str(base[i]), int(meta['n0'][i]), int(meta['n1'][i]), i), t))
        mo = {'sign_test': recs, 'window': (a.window - 1) // 2, 'WindOvlp': a.WindOvlp, 'percentile': a.percentile, 'NA': a.NA}
        ranked = detect.region_rank(mo, 2 if method == 'ks' else 3, 1 if a.rankUse == 'pv' else 0)
        order = np.array([r[0][6] for r in ranked], dtype=np.int64)
    return meta, res, order


def rank_order(res, method, rank_use, device=0):
    """myDetect.py:447-462: stable ascending sort by (combined, KS, MWU) p-value (or statistic, reversed)."""
    pind = 'p' if rank_use == 'pv' else 'st'
    first = ('comb_p' if pind == 'p' else 'comb_st') if method != 'ks' else ('ks_p' if pind == 'p' else 'ks_d')
    return engine.rank_order_host(res[first], res['ks_p' if pind == 'p' else 'ks_d'], res['mwu_p' if pind == 'p' else 'mwu_u'],
                                  descending=(rank_use == 'st'), device=device)


def write_sign_test(path, meta, res, with_comb):
    engine.write_sign_test_host(path, meta, res, with_comb)


def main(argv=None):
    parser = build_parser()
    a = parser.parse_args(argv)
    if a.cmd == 'readclasses':
        errs = validate_readclasses(a)
        if errs:
            print('\n'.join(errs))
            return 1
        run_readclasses(a)
        return 0
    if a.cmd == 'readhmm':
        errs = validate_readhmm(a)
        if errs:
            print('\n'.join(errs))
            return 1
        run_readhmm(a)
        return 0
    if a.cmd == 'readpairs':
        errs = validate_readpairs(a)
        if errs:
            print('\n'.join(errs))
            return 1
        run_readpairs(a)
        return 0
    if a.cmd == 'readdiff':
        errs = validate_readdiff(a)
        if errs:
            print('\n'.join(errs))
            return 1
        run_readdiff(a)
        return 0
    if a.cmd == 'readllr':
        errs = validate_readllr(a)
        if errs:
            print('\n'.join(errs))
            return 1
        run_readllr(a)
        return 0
    if a.cmd == 'readcalls':
        errs = validate_readcalls(a)
        if errs:
            print('\n'.join(errs))
            return 1
        run_readcalls(a)
        return 0
    if a.cmd == 'rescale':
        errs = validate_rescale(a)
        if errs:
            print('\n'.join(errs))
            return 1
        run_rescale(a)
        return 0
    if a.cmd == 'kmermix':
        errs = validate_kmermix(a)
        if errs:
            print('\n'.join(errs))
            return 1
        run_kmermix(a)
        return 0
    if a.cmd in ('kmermodel', 'kmerprofile'):
        errs = validate_kmer(a)
        if errs:
            print('\n'.join(errs))
            return 1
        run_kmermodel(a) if a.cmd == 'kmermodel' else run_kmerprofile(a)
        return 0
    if a.cmd in ('profile', 'detect1'):
        errs = validate1(a)
        if errs:
            print('\n'.join(errs))
            return 1
        if a.cmd == 'profile':
            run_profile(a)
            return 0
        meta, res, order = run_detect1(a)
        first = ('comb_p' if a.testMethod != 'ks' else 'ks_p')
        for r, i in enumerate(order[:a.topN]):
            print('%d %s %s %d %s %.3E' % (r + 1, meta['chrom'][i], meta['strand'][i], meta['pos'][i] + 1, meta['base'][i], res[first][i]))
        return 0
    if a.cmd != 'detect':
        parser.print_help()
        return 1
    errs = validate(a)
    if errs:
        print('\n'.join(errs))
        parser.parse_args(['detect', '-h']) if False else None
        return 1
    meta, res, order = run_detect(a)
    top = order[:a.topN]
    first = ('comb_p' if a.testMethod != 'ks' else 'ks_p')
    for r, i in enumerate(top):
        print('%d %s %s %d %s %.3E' % (r + 1, meta['chrom'][i], meta['strand'][i], meta['pos'][i] + 1, meta['base'][i],
                                       res[first][i]))
    return 0


if __name__ == '__main__':
    sys.exit(main())
