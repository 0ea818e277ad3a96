"""What tests/test_estimator_cases_cpu.py and tests/test_estimator_edges_gpu.py share beyond the inputs of
tests/estimator_cases.py: the seeded module whose weights a case runs with, the float64 yardstick's result on a case, and
the float32 evaluation that sets the numeric tolerance.

THE TOLERANCE.  tests/test_estimator_gpu.py allows 4 x the reference's own float32 distance from float64, measured on its
fixture.  For generated inputs the same quantity is measured here on a float32 evaluation of the same precision class, never
on the kernel: the module's own torch layers on the CPU in float32 (``iou_estimator`` -> per-box ``amax`` -> ``iou_head``
-> sigmoid) on ``EN.features`` cast to float32.  ``e32_iou`` / ``e32_pooled`` = its largest distance from the float64
values over the case's survivors; the GPU test's gate is 4 x that."""
import functools

import numpy as np
import torch
from torch import nn

import estimator_cases as EC
import estimator_numpy as EN


@functools.lru_cache(maxsize=None)
def module(classes):
    """``build_estimator`` for tasks of ``classes`` classes each, seeded as tools/gen_golden_estimator.py seeds its own:
    ``torch.manual_seed``, then non-identity BatchNorm statistics from a seeded generator.  On the CPU, in eval mode."""
    from al3d.models import build_estimator
    tasks = [dict(num_class=n, class_names=[f"t{t}c{k}" for k in range(n)]) for t, n in enumerate(classes)]
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(20)
        m = build_estimator(dict(type="Estimator", tasks=tasks, dim_feat=224))
    g = torch.Generator().manual_seed(21)
    for mod in m.modules():
        if isinstance(mod, nn.BatchNorm1d):
            mod.weight.data = torch.rand(mod.num_features, generator=g) + 0.5
            mod.bias.data = torch.randn(mod.num_features, generator=g) * 0.1
            mod.running_mean.data = torch.randn(mod.num_features, generator=g) * 0.2
            mod.running_var.data = torch.rand(mod.num_features, generator=g) * 1.5 + 0.5
    return m.eval()


def state(classes):
    return {k: v.detach().numpy().copy() for k, v in module(classes).state_dict().items()}


@functools.lru_cache(maxsize=None)
def yardstick(name):
    """``EN.run`` on the case (float64), plus ``f32_iou`` / ``f32_pooled`` (the float32 torch evaluation, per input slot,
    NaN / 0 where no point) and ``e32_iou`` / ``e32_pooled``.  Computed once per process; read-only."""
    c = EC.case(name)
    with np.errstate(invalid="ignore"):
        y = EN.run(c["boxes"], c["labels"], c["counts"], c["points"], c["offsets"], state(c["classes"]), c["num_classes"],
                   c["rot_col"])
    B, nt, post = c["labels"].shape
    m = module(c["classes"])
    rows, owner = [], []
    for b in range(B):
        pts = c["points"][c["offsets"][b]:c["offsets"][b + 1]]
        slots, mask = c["hits"][b]
        for k, s in enumerate(slots):
            if mask[k].any():
                t, i = divmod(s, post)
                rows.append(EN.features(pts[mask[k]], c["boxes"][b, t, i], c["labels"][b, t, i], c["num_classes"], c["rot_col"]))
                owner.append((b, t, i))
    f32_iou = np.full((B, nt, post), np.nan, dtype=np.float32)
    f32_pooled = np.zeros((B, nt, post, 128), dtype=np.float32)
    with torch.no_grad():
        per_point = m.iou_estimator(torch.from_numpy(np.concatenate(rows).astype(np.float32)))
        pooled = torch.stack([x.amax(0) for x in torch.split(per_point, [len(r) for r in rows])])
        iou = torch.sigmoid(m.iou_head(pooled))[:, 0]
    for k, (b, t, i) in enumerate(owner):
        f32_iou[b, t, i], f32_pooled[b, t, i] = iou[k].item(), pooled[k].numpy()
    idx = tuple(np.array(owner).T)
    y.update(f32_iou=f32_iou, f32_pooled=f32_pooled, owners=owner,
             e32_iou=float(np.abs(f32_iou[idx].astype(np.float64) - y["iou"][idx]).max()),
             e32_pooled=float(np.abs(f32_pooled[idx].astype(np.float64) - y["pooled"][idx]).max()))
    return y
