"""The exact integers K1 leaves in the workspace for K2 (nanomod_amd/csrc/rank_stats.hpp: ks_num, mwu_s, tie), from their
definitions, and a reader of those three arrays out of a DeviceDetector's workspace tensor.  Shared by test_hist_model.py
(CPU: the reference against the two oracles) and test_rank_hist_constructed_gpu.py."""
import numpy as np

KS_D_FLOAT_FORM_ABS = 4.5e-16     # the project's bound between ks_2samp's float form of D and the correctly rounded rational


def exact_ints(a, b):
    """(ks_num, mwu_s, tie) of group 1 = a, group 2 = b as Python integers:
    ks_num = max over the pooled points v of |#{a <= v} * n1 - #{b <= v} * n0|
    mwu_s  = sum over x in a of (#{b < x} + #{b <= x})
    tie    = sum over the pooled tie groups of t^3 - t
    Comparisons are numpy's: -0.0 == +0.0."""
    a = np.sort(np.asarray(a, dtype=np.float64)); b = np.sort(np.asarray(b, dtype=np.float64))
    n0, n1 = int(a.shape[0]), int(b.shape[0])
    pooled, counts = np.unique(np.concatenate([a, b]), return_counts=True)
    c0 = np.searchsorted(a, pooled, side='right'); c1 = np.searchsorted(b, pooled, side='right')
    ks_num = max(abs(int(x) * n1 - int(y) * n0) for x, y in zip(c0, c1)) if n0 and n1 else 0
    mwu_s = int(np.searchsorted(b, a, side='left').sum()) + int(np.searchsorted(b, a, side='right').sum())
    tie = sum(int(t) ** 3 - int(t) for t in counts)
    return ks_num, mwu_s, tie


def mwu_u_of(mwu_s, n0, n1):
    """scipy's statistic min(U1, U2), U1 = n0 n1 + n0 (n0 + 1) / 2 - (rank sum of group 1) = n0 n1 - mwu_s / 2"""
    u1 = n0 * n1 - mwu_s / 2.0
    return min(u1, n0 * n1 - u1)


def align256(x):
    return (x + 255) & ~255


class WorkspaceLayoutMoved(AssertionError):
    pass


def read_k1_ints(det, npos, res=None, n0=None, n1=None, rational_d=False, ks_num_written=True):
    """ks_num (uint32), mwu_s and tie (uint64) of the detector's last device-resident run(), all tests, over `npos` positions:
    the first three take() calls of carve() in nanomod_hip.hip — offsets 0, align256(4 npos), + align256(8 npos).

    res / n0 / n1: the same call's outputs (CUDA tensors or numpy arrays) and the group sizes.  What was read must reproduce them,
    or the workspace layout moved and WorkspaceLayoutMoved is raised instead of a wrong answer:
      mwu_u == min(u1, n0 n1 - u1), u1 = n0 n1 - mwu_s / 2             (positions without NMOD_STATUS_MWU_ALL_IDENTICAL; a KS-only
               run has no mwu_u track and writes neither mwu_s nor tie: only ks_num is checked, and only it means anything)
      ks_d  == ks_num / (n0 n1) correctly rounded with rational_d (NMOD_FLAG_KS_RATIONAL_D in effect: KS-only batches), else
               within the project's 4.5e-16 of it (the float form |fl(c0/n0) - fl(c1/n1)|).
    ks_num_written: rank_pair_kernel evaluates the float form only and writes no ks_num — False leaves that array unchecked."""
    det.torch.cuda.synchronize()
    ws = det._ws
    o_mwu = align256(4 * npos)
    o_tie = o_mwu + align256(8 * npos)
    assert ws is not None and ws.numel() >= o_tie + 8 * npos
    host = ws[:o_tie + 8 * npos].cpu().numpy()
    ks_num = host[:4 * npos].view(np.uint32).copy()
    mwu_s = host[o_mwu:o_mwu + 8 * npos].view(np.uint64).copy()
    tie = host[o_tie:o_tie + 8 * npos].view(np.uint64).copy()
    if res is not None:
        get = lambda k: res[k].cpu().numpy() if hasattr(res[k], 'cpu') else np.asarray(res[k])
        n0 = np.asarray(n0, dtype=np.int64); n1 = np.asarray(n1, dtype=np.int64)
        prod = (n0 * n1).astype(np.float64)
        live = (get('status') & 1) == 0
        u1 = prod - mwu_s.astype(np.float64) / 2.0
        if 'mwu_u' in res and not np.array_equal(np.minimum(u1, prod - u1)[live], get('mwu_u')[live]):
            raise WorkspaceLayoutMoved('the workspace layout moved: mwu_s as read does not reproduce mwu_u (carve() in nanomod_hip.hip)')
        if ks_num_written:
            d = ks_num.astype(np.float64) / prod
            ok = np.array_equal(d, get('ks_d')) if rational_d else bool(np.all(np.abs(d - get('ks_d')) <= KS_D_FLOAT_FORM_ABS))
            if not ok:
                raise WorkspaceLayoutMoved('the workspace layout moved: ks_num as read does not reproduce ks_d (carve() in nanomod_hip.hip)')
    return {'ks_num': ks_num, 'mwu_s': mwu_s, 'tie': tie}
