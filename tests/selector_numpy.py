"""Independent yardstick for the selection operators: each one stated with the very numpy /
torch-CPU calls the reference makes, so NaN, inf and signed zeros behave as they do there.

Nothing here imports ``oracle`` or ``al3d``.  The HIP kernels (tests/test_selector_edges_gpu.py)
and the C oracle (tests/test_selector_edges_cpu.py) are both compared against this file; the
oracle and the kernels were written by one hand, this file is what keeps the two from agreeing
with each other on a misreading of ``argmax``, ``min(0)`` or ``argsort``.

Reference lines are paths relative to the reference repository.
"""
import numpy as np
import torch


# ---------------------------------------------------------------- greedy k-center loop
def greedy(D, seeded, first, box_cost, cost_f, start_cost, budget_int, seed_map=None,
           check_seeded=False, cap=None):
    """The pick loop of det3d/selectors/badge_selector.py:148-176 (float32, torch),
    spatial_temporal_selector.py:160-190 (float64, numpy) and ppal_selector.py:210-235.

    float32 maps run through ``torch.stack(..).min(0)[0]`` / ``torch.argmax``, float64 maps
    through ``np.stack(..).min(0)`` / ``np.argmax``, as in the reference.  Returns
    ``(status, picks)``: 0, or -1 with the picks made so far where the reference's
    ``assert selected_index not in selected_index_list`` fires (``check_seeded`` extends the
    assert to the seeded list, as the spatial / temporal selectors do), or -2 when ``cap`` picks
    are made and one more would fit the budget.
    """
    assert D.dtype in (np.float32, np.float64)
    n = D.shape[0]
    seed_map = D if seed_map is None else seed_map
    seeded = [int(s) for s in seeded]
    cap = n + 1 if cap is None else cap
    if D.dtype == np.float32:
        Dm, Sm = torch.from_numpy(D), torch.from_numpy(np.ascontiguousarray(seed_map))
        stack_min = lambda rows: torch.stack(rows).min(0)[0]
        argmax = lambda v: int(torch.argmax(v))
    else:
        Dm, Sm = D, seed_map
        stack_min = lambda rows: np.stack(rows).min(0)
        argmax = lambda v: int(np.argmax(v))
    if seeded:
        fps = stack_min([Sm[i] for i in seeded])
        picks = [argmax(fps)]
    else:
        picks = [int(first)]
        fps = Sm[picks[-1]]
    cost = start_cost
    cost += cost_f
    cost += box_cost[picks[-1]]
    while True:
        fps = stack_min([fps, Dm[picks[-1]]])
        sel = argmax(fps)
        if sel in picks or (check_seeded and sel in seeded):
            return -1, picks
        cost += cost_f
        cost += box_cost[sel]
        if cost > budget_int:
            return 0, picks
        if len(picks) >= cap:
            return -2, picks
        picks.append(sel)


# ---------------------------------------------------------------- uncertainty operators
def argsort_desc(x):
    """entropy_selector.py:121 ``torch.argsort(-x)``, made deterministic with ``stable=True``."""
    return torch.argsort(-torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)), stable=True).numpy()


def argsort_desc_numpy(x):
    return np.argsort(-np.asarray(x, dtype=np.float32), kind="stable")


def minmax_norm(x):
    """uwe_selector.py:78."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return ((t - t.min()) / (t.max() - t.min())).numpy()


def scale_rows(feats, w, widx=None):
    """badge_selector.py:75-78, uwe_selector.py:96-99: ``feats * w[:, None]``; with an index
    vector the weight of row i is ``w[widx[i]]``."""
    w = np.asarray(w, dtype=np.float32)
    if widx is not None:
        w = w[np.asarray(widx, dtype=np.int64)]
    return np.asarray(feats, dtype=np.float32) * w[:, None]


def _binary_entropy(s):
    return -s * torch.log(s) - (1.0 - s) * torch.log(1 - s)


def _kept(a, counts, b):
    return torch.from_numpy(np.concatenate([a[b, t, :counts[b, t]] for t in range(a.shape[1])]))


def frame_entropy(scores, counts):
    """entropy_selector.py:72-75: mean binary entropy of a frame's kept scores; the mean of an
    empty tensor is NaN."""
    return np.array([float(_binary_entropy(_kept(scores, counts, b)).mean())
                     for b in range(scores.shape[0])], dtype=np.float32)


def frame_weighted_entropy(scores, labels, counts, class_weight):
    """ppal_selector.py:99-109: sum of entropy * class_weight[label]; an empty frame sums to 0.
    A label outside the weight table raises IndexError here, as it does in the reference."""
    cw = torch.from_numpy(np.ascontiguousarray(class_weight, dtype=np.float32))
    out = []
    for b in range(scores.shape[0]):
        h = _binary_entropy(_kept(scores, counts, b))
        out.append(float((h * cw[_kept(labels, counts, b).long()]).sum()))
    return np.array(out, dtype=np.float32)


def mask_map(D, keep):
    """ppal_selector.py:194-196 (the two ``= -np.inf`` assignments)."""
    out = np.array(D, dtype=np.float32, copy=True)
    keep = np.asarray(keep, dtype=bool)
    out[~keep] = -np.inf
    out[:, ~keep] = -np.inf
    return out


def l1_map(feats, p):
    """feature_selector.py:87-109: row i is ``torch.abs(feats - feats[i]).sum(1)`` for p == 1 and
    ``torch.sqrt((feats - feats[i]) ** 2).sum(1)`` for p == 2."""
    f = torch.from_numpy(np.ascontiguousarray(feats, dtype=np.float32))
    out = torch.zeros([f.shape[0], f.shape[0]])
    for i in range(f.shape[0]):
        out[i] = torch.abs(f - f[i]).sum(1) if p == 1 else torch.sqrt((f - f[i]) ** 2).sum(1)
    return out.numpy()


def euclid_map(xy, loc_id):
    """euclidean_spatial_selector.py:95-106: sqrt(dx*dx + dy*dy) inside one map location, 1e6
    across locations."""
    xy = np.asarray(xy, dtype=np.float64)
    loc_id = np.asarray(loc_id)
    dx = xy[None, :, 0] - xy[:, None, 0]
    dy = xy[None, :, 1] - xy[:, None, 1]
    out = np.sqrt(dx * dx + dy * dy)
    out[loc_id[:, None] != loc_id[None, :]] = 1e6
    return out
