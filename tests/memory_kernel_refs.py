"""Plain float64 statements of the memory readout, usage and consolidation operations, and the a-priori round-off bounds
the GPU tests hold the kernels to.

Written from the header comments of include/xmem_hip.h and from the oracle (oracle/cpu_ref.py), not from the kernels.
Row-major operands, as the C ABI takes them: memory rows [n, C], weights / indices [HW, top_k], similarity [P, n].
tests/test_memory_kernel_refs_host.py ties every function here to the oracle on the CPU; tests/test_gpu_memory_kernels.py
compares the kernels with them.
"""
import numpy as np
import torch

from oracle import cpu_ref as R

U = 2.0 ** -24            # unit round-off of fp32 (round to nearest)


def _np64(t):
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.asarray(t, dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------
# readout and usage
# ---------------------------------------------------------------------------------------------------------
def readout_ref(vsegs, w, idx):
    """out[obj][q][c] = sum_s w[q][s] * V_obj[idx[q][s]][c], V_obj = the object's segments concatenated (None / empty
    segments contribute no rows).  vsegs[obj][seg]: [n_seg, Cv] | None; w, idx: [HW, top_k].
    Returns (value, magnitude), both float64 [n_obj, HW, Cv]; magnitude = sum_s |w| |v|."""
    w = _np64(w)
    idx = np.asarray(idx.cpu() if isinstance(idx, torch.Tensor) else idx).astype(np.int64)
    vals, mags = [], []
    for segs in vsegs:
        V = np.concatenate([_np64(s) for s in segs if s is not None and s.shape[0] > 0], 0)
        rows = V[idx]                                          # [HW, k, Cv]
        vals.append((w[:, :, None] * rows).sum(1))
        mags.append((np.abs(w)[:, :, None] * np.abs(rows)).sum(1))
    return np.stack(vals, 0), np.stack(mags, 0)


def usage_ref(w, idx, first, count):
    """usage = affinity.sum(dim=2) restricted to elements [first, first + count) of the index space, from the sparse
    affinity (w, idx).  Returns (sum float64 [count], hits int64 [count])."""
    w = _np64(w).reshape(-1)
    idx = np.asarray(idx.cpu() if isinstance(idx, torch.Tensor) else idx).astype(np.int64).reshape(-1)
    inside = (idx >= first) & (idx < first + count)
    S = np.zeros(count, np.float64)
    hits = np.zeros(count, np.int64)
    np.add.at(S, idx[inside] - first, w[inside])
    np.add.at(hits, idx[inside] - first, 1)
    return S, hits


def usage_bound(S, hits, use_old):
    """2 * (hits * 2^-40 + u * S + u * |use_old + S|): truncation at 2^-40 per term, one rounding of the sum, one rounding of
    the add; the factor 2 covers second-order terms."""
    return 2.0 * (hits * 2.0 ** -40 + U * S + U * np.abs(_np64(use_old) + S))


# ---------------------------------------------------------------------------------------------------------
# eviction / prototype selection
# ---------------------------------------------------------------------------------------------------------
def topk_1d_ref(v, k, largest=True):
    """torch.topk(v, k, largest, sorted=True) with the documented tie rule: among equal values the lower index first
    (-0.0 == +0.0).  Returns (values float32 [k], indices int64 [k])."""
    v = np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v, dtype=np.float32).reshape(-1)
    if not 1 <= k <= v.size:
        raise ValueError('k out of range')
    order = np.argsort(-v if largest else v, kind='stable')[:k]
    return v[order], order.astype(np.int64)


def select_greater_ref(usage, threshold):
    """Indices i with usage[i] > threshold, ascending."""
    usage = np.asarray(usage.cpu() if isinstance(usage, torch.Tensor) else usage, dtype=np.float32).reshape(-1)
    return np.nonzero(usage > np.float32(threshold))[0].astype(np.int64)


# ---------------------------------------------------------------------------------------------------------
# consolidation
# ---------------------------------------------------------------------------------------------------------
def softmax_suffix_ref(sim, count):
    """Softmax (with max shift) over the last `count` entries of each row of sim [P, n], zeros before.  float64."""
    x = _np64(sim)
    n = x.shape[1]
    out = np.zeros_like(x)
    t = x[:, n - count:]
    e = np.exp(t - t.max(1, keepdims=True))
    out[:, n - count:] = e / e.sum(1, keepdims=True)
    return out


def softmax_suffix_rel_bound(sim, count, lib_factor=1.0):
    """Relative bound per row: (A + count/256 + 16) * u, A = the row's largest (rowmax - x) among entries whose float64
    result exceeds 1e-30 (the rounding of the shifted argument is amplified by its size)."""
    x = _np64(sim)
    n = x.shape[1]
    t = x[:, n - count:]
    ref = softmax_suffix_ref(sim, count)[:, n - count:]
    d = t.max(1, keepdims=True) - t
    A = np.where(ref > 1e-30, d, 0.0).max(1, keepdims=True)
    return lib_factor * (A + count / 256.0 + 16.0) * U


def weighted_rows_ref(aff, count, V):
    """out[p][c] = sum_i aff[p][n - count + i] * V[i][c].  Returns (value, magnitude = sum_i |aff| |V|), float64 [P, C]."""
    a = _np64(aff)
    V = _np64(V)
    if V.ndim == 1:
        V = V[:, None]
    a = a[:, a.shape[1] - count:]
    return a @ V, np.abs(a) @ np.abs(V)


def similarity_dense_ref(key, shrinkage, qk, qe):
    """Anisotropic L2 similarity of key [n, Ck] (shrinkage [n] | None) against P queries qk / qe [P, Ck] (qe | None):
    the oracle's get_similarity on float64 inputs.  Returns float64 [P, n]."""
    d = lambda t: torch.as_tensor(t).detach().cpu().double()
    mk = d(key).t().unsqueeze(0)
    ms = d(shrinkage).view(1, 1, -1) if shrinkage is not None else None
    k = d(qk).t().unsqueeze(0)
    e = d(qe).t().unsqueeze(0) if qe is not None else None
    return R.get_similarity(mk, ms, k, e)[0].t().contiguous().numpy()


def similarity_dense_bound(key, shrinkage, qk, qe):
    """(2 Ck + 4) u (sum_c (|x^2 e| + 2 |x k e|) + |b_sq|) ms / sqrt(Ck) per element [P, n]."""
    x, k = _np64(key), _np64(qk)
    ck = x.shape[1]
    e = _np64(qe) if qe is not None else np.ones_like(k)
    mag = (x * x) @ np.abs(e).T + 2.0 * np.abs(x) @ np.abs(k * e).T            # [n, P]
    if qe is not None:
        mag = mag + np.abs((e * k * k).sum(1))[None, :]
    ms = np.abs(_np64(shrinkage))[:, None] if shrinkage is not None else 1.0
    return ((2 * ck + 4) * U * mag * ms / np.sqrt(ck)).T


def consolidation_ref(cand_key, cand_shr, cand_sel, usage, cand_values, P, return_aux=False):
    """RefMemory.consolidation (oracle/cpu_ref.py) in float64, reference-shaped operands: cand_key / cand_sel [1, Ck, n],
    cand_shr [1, 1, n], usage [1, 1, n] (fp32: the ranking is on the fp32 usage), cand_values[g] [n_obj, Cv, n_g] | None.
    The prototype choice goes through topk_1d_ref (ties -> lower index first; torch.topk leaves that order open).
    Returns (proto_key [1, Ck, P], proto_value list, proto_shrinkage [1, 1, P] | None) (+ a dict of intermediates)."""
    d = lambda t: t.detach().cpu().double() if t is not None else None
    cand_key, cand_shr, cand_sel = d(cand_key), d(cand_shr), d(cand_sel)
    cand_values = [d(gv) for gv in cand_values]
    n = cand_key.shape[-1]
    _, order = topk_1d_ref(usage.detach().cpu().float().flatten(), P, largest=True)
    proto_idx = torch.from_numpy(order)
    validity = [proto_idx >= (n - gv.shape[2]) if gv is not None else None for gv in cand_values]
    proto_key = cand_key[:, :, proto_idx]
    proto_sel = cand_sel[:, :, proto_idx] if cand_sel is not None else None
    similarity = R.get_similarity(cand_key, cand_shr, proto_key, proto_sel)                    # [1, n, P]
    affinity = [R.do_softmax(similarity[:, -gv.shape[2]:, validity[gi]]) if gv is not None else None
                for gi, gv in enumerate(cand_values)]
    affinity = [a if a is None or a.shape[-1] > 0 else None for a in affinity]
    proto_value = [gv @ affinity[gi] if affinity[gi] is not None else None for gi, gv in enumerate(cand_values)]
    proto_shr = cand_shr @ affinity[0] if cand_shr is not None else None
    if return_aux:
        return proto_key, proto_value, proto_shr, dict(proto_idx=proto_idx, validity=validity, similarity=similarity,
                                                       affinity=affinity, proto_sel=proto_sel)
    return proto_key, proto_value, proto_shr
