"""GPU suite of the BEV map segmentation head (csrc/bev_seg.hip, al3d/models/bev_seg_head.py) against the float64
yardstick (tests/bev_seg_fp64.py): the grid resample, the classifier kernel with its reductions, the argument contract of
both entry points, the head module and the camera-only detector with a map head.

BOUNDS.  u = 2^-24.
  * Resample: 6 u x (sum |w||v|), not the 8 u the blend could be allowed: in r0 (c0 v00 + c1 v01) + r1 (c0 v10 + c1 v11) a
    term passes the rounding of its column weight, the product, the inner sum, the rounding of its row weight, the
    product and the outer sum -- six roundings (first order; the factor 1 / (1 - 6 u) covers the rest).
  * Classifier probabilities: 0.25 (C + 2) u (sum |w||x| + |b|) + the sigmoid's own error; entropy of a pixel: 0.2240
    (the largest slope |z| p (1 - p) of the entropy in the logit) times the same logit bound + the entropy's own error; the
    per-frame sum: the sum of the pixels' bounds + (25 + ceil(workgroups / 16)) u x the sum, the depth of the fixed-order
    summation: six butterfly steps over a wave's 64 pixels, three adds over the waves of a 256-pixel workgroup,
    ceil(workgroups / 16) adds per slot of the second pass, 16 adds over the slots.
  * The kernel's own sigmoid and entropy errors are MEASURED on the GPU against float64 over logits planted exactly
    (a one-channel input, weight 1, bias 0; 8,192 logits across [-30, 30] and the points below) and allowed 4 x:

        MEASURED   sigmoid 8.8e-08   entropy 1.1e-06      (max absolute error, one MI355X: 8.711e-08 / 1.048e-06)
        TIGHT_MAX  sigmoid 3.52e-07  entropy 4.4e-06      (4 x MEASURED)

    The entropy's figure is that of the stated formula on the ROUNDED p: near p = 1 an ulp of p (6e-8) times the slope
    ln((1 - p) / p) (up to 16.6 before p rounds to 1) is 1e-6.

    HOW TO RE-RECORD: run test_sigmoid_and_entropy_own_error with -s, copy the printed maxima rounded up to two digits
    into MEASURED below and here; TIGHT_MAX follows.  The test fails when a fresh maximum exceeds TIGHT_MAX.
  * area differs from the yardstick's at most by the pixels whose float64 probability lies within the probability bound
    of 0.5, and those are under 1 % of the pixels (the same seeds are checked on the CPU in tests/test_bev_seg_cpu.py).
  * Head: logits within (2 E_MAX + 6 u + (C + 2) u) x the abs-chain normaliser -- dense_fp64.E_MAX for each of the two
    split-arithmetic 3x3 layers, the resample's and the classifier's f32 bounds above, every layer's error carried to the
    logits by the abs chain of the layers behind it -- hence probabilities within a quarter of that + the sigmoid's.

Measured on one MI355X: resample 3.1 / 2.4 / 3.5 u of the normaliser at C = 32 / 4 / 256; classifier probabilities 9.1e-08 ..
2.0e-07 (at most 3.6 % of the bound), entropy sums 4.5e-06 .. 1.9e-05 (at most 1.4 %); head 1.2e-07 (0.2 % of the bound) under
all three arithmetics; detector head 3.4e-06.  Also in DESIGN 8e."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bev_seg_fp64 as Y
from test_bev_seg_cpu import CLASSIFY_CASES, classify_case, golden, prob_bound, scopes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURED = dict(sigmoid=8.8e-08, entropy=1.1e-06)
TIGHT_MAX = {k: 4.0 * v for k, v in MEASURED.items()}
ENT_SLOPE = 0.2240
_REF = {}


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------ resample
def resample_case(C):
    """The golden's map (C = 32, B = 2) or a seeded one of the same size with C channels and N = 1; its float64 resample and
    normaliser, computed once."""
    if ("resample", C) not in _REF:
        g = golden()
        i_s, o_s = scopes(g["cfg"])
        x = g["x"] if C == 32 else torch.randn(1, C, 12, 20, generator=torch.Generator().manual_seed(C))
        _REF["resample", C] = dict(x=x, i_s=i_s, o_s=o_s, ref=nhwc(Y.resample64(x, i_s, o_s)),
                                   norm=nhwc(Y.resample64(x, i_s, o_s, absolute=True)),
                                   mask=Y.padded_mask(i_s, o_s, x.shape[-2:]))
    return _REF["resample", C]


@pytest.mark.parametrize("C", [32, 4, 256])
def test_resample_against_the_yardstick(C):
    from al3d import detector_ops as D
    c = resample_case(C)
    src = nhwc(c["x"]).to(DEV)
    got = D.bev_grid_resample_nhwc(src, c["i_s"], c["o_s"])
    assert tuple(got.shape) == tuple(c["ref"].shape) == (c["x"].shape[0], 20, 23, C)
    err = (got.cpu().double() - c["ref"]).abs()
    bound = 6.0 * Y.U / (1.0 - 6.0 * Y.U) * c["norm"]
    live = c["norm"] > 0
    print(f"C={C}: max err {float(err.max()):.3e}, max err / (u x normaliser) {float((err[live] / (Y.U * c['norm'][live])).max()):.3f} (bound 6)")
    assert bool((err <= bound).all())
    assert bool(c["mask"].any()) and bool((got.cpu()[:, c["mask"]] == 0).all())           # zero padding: exactly 0
    # NaN in the map does not reach a padded output either: an outside tap is dropped, not multiplied by zero
    poisoned = src.clone()
    poisoned[:, 0, :, :] = float("nan")
    poisoned[:, :, 0, :] = float("nan")
    assert bool((D.bev_grid_resample_nhwc(poisoned, c["i_s"], c["o_s"]).cpu()[:, c["mask"]] == 0).all())
    swapped = D.bev_grid_resample_nhwc(src, c["i_s"], c["o_s"], out_hw_swapped=True)
    assert tuple(swapped.shape) == (c["x"].shape[0], 23, 20, C) and torch.equal(swapped, got.permute(0, 2, 1, 3).contiguous())


# ------------------------------------------------------------------ classifier
def planted_logits():
    """float32 logits planted exactly: 8,192 across [-30, 30], the ends of the sigmoid's float32 range and points about 0."""
    extra = torch.tensor([0.0, -2.0 ** -21, 2.0 ** -21, -1e-3, 1e-3, 16.6, 16.7, 17.4, -87.0, -88.5, -89.5, -104.0, 88.0, 100.0])
    return torch.cat([torch.linspace(-30.0, 30.0, 8192), extra])


def test_sigmoid_and_entropy_own_error():
    """One pixel per frame, one channel carrying the logit (weight 1, bias 0: the FMA chain and the butterfly add zeros,
    so the kernel's logit IS the planted one); entropy_sum of a one-pixel frame is the pixel's entropy."""
    from al3d import detector_ops as D
    z = planted_logits()
    x = torch.zeros(len(z), 1, 1, 4)
    x[:, 0, 0, 0] = z
    w = torch.tensor([[1.0, 0.0, 0.0, 0.0]])
    prob, ent, area = D.seg_classify(x.to(DEV), w.to(DEV), torch.zeros(1, device=DEV), with_stats=True)
    p, e = prob.cpu().double().view(-1), ent.cpu().double().view(-1)
    p64, e64 = Y.sigmoid64(z), Y.entropy64(z)
    ep, ee = float((p - p64).abs().max()), float((e - e64).abs().max())
    print(f"own error over {len(z)} planted logits: sigmoid {ep:.3e}, entropy {ee:.3e} "
          f"(recorded MEASURED {MEASURED['sigmoid']:.1e} / {MEASURED['entropy']:.1e})")
    assert ep <= TIGHT_MAX["sigmoid"] and ee <= TIGHT_MAX["entropy"]
    # the entropy is exactly 0 where p rounds to 0 or 1, and only there
    ends = (prob.cpu().view(-1) == 0) | (prob.cpu().view(-1) == 1)
    assert bool(ends.any()) and bool((ent.cpu().view(-1)[ends] == 0).all()) and bool((ent.cpu().view(-1)[~ends] > 0).all())
    assert torch.equal(area.cpu().view(-1).long(), (prob.cpu().view(-1) > 0.5).long())
    assert bool((area.cpu().view(-1)[z > 1e-4] == 1).all()) and bool((area.cpu().view(-1)[z <= 0] == 0).all())


def classify_ref(case):
    if ("classify", case) not in _REF:
        x, w, b = classify_case(*case)
        z = Y.logits64(x.permute(0, 3, 1, 2), w, b)
        _REF["classify", case] = dict(x=x, w=w, b=b, z=z, p=Y.sigmoid64(z), e=Y.entropy64(z), bound=prob_bound(x, w, b))
    return _REF["classify", case]


@pytest.mark.parametrize("case", CLASSIFY_CASES)
def test_classify_against_the_yardstick(case):
    from al3d import detector_ops as D, lib
    from al3d.selector_ops import _ptr, _stream
    C, K, N, H, W = case
    assert (H * W) % 256 and H != W and H * W > 256
    c = classify_ref(case)
    x, w, b = c["x"].to(DEV), c["w"].to(DEV), c["b"].to(DEV)
    prob, ent, area = D.seg_classify(x, w, b, with_stats=True)
    assert tuple(prob.shape) == (N, K, H, W) and tuple(ent.shape) == tuple(area.shape) == (N, K) and area.dtype == torch.int32
    perr = (prob.cpu().double() - c["p"]).abs()
    pb = c["bound"] + TIGHT_MAX["sigmoid"]
    print(f"{case}: prob max err {float(perr.max()):.3e}, max err / bound {float((perr / pb).max()):.3f}")
    assert bool((perr <= pb).all())
    groups = -(-H * W // 256)
    esum = c["e"].sum((-2, -1))
    eb = (4.0 * ENT_SLOPE * c["bound"] + TIGHT_MAX["entropy"]).sum((-2, -1)) + (25 + -(-groups // 16)) * Y.U * esum
    eerr = (ent.cpu().double() - esum).abs()
    print(f"{case}: entropy sum max err {float(eerr.max()):.3e}, max err / bound {float((eerr / eb).max()):.3f}")
    assert bool((eerr <= eb).all())
    near = ((c["p"] - 0.5).abs() <= pb).sum((-2, -1))
    assert float(near.sum()) / c["p"].numel() < 0.01
    assert bool(((area.cpu().long() - (c["p"] > 0.5).sum((-2, -1))).abs() <= near).all())
    assert torch.equal(area.cpu().long(), (prob.cpu() > 0.5).sum((-2, -1)))
    # two runs: identical bits, all three outputs
    prob2, ent2, area2 = D.seg_classify(x, w, b, with_stats=True)
    assert torch.equal(prob, prob2) and torch.equal(ent.view(torch.int32), ent2.view(torch.int32)) and torch.equal(area, area2)
    # null entropy_sum / area pointers: the probabilities do not change, the other reduction neither
    assert torch.equal(D.seg_classify(x, w, b), prob)
    ws = torch.empty(int(lib.load().al3d_seg_classify_workspace_bytes(N, H, W)), dtype=torch.uint8, device=DEV)
    for want_ent, want_area in ((True, False), (False, True)):
        p3 = torch.full_like(prob, -1.0)
        e3, a3 = torch.full_like(ent, -1.0), torch.full_like(area, -1)
        lib.call("al3d_seg_classify_f32", _ptr(x), _ptr(w), _ptr(b), N, H, W, C, K, _ptr(p3), _ptr(e3) if want_ent else None,
                 _ptr(a3) if want_area else None, _ptr(ws), _stream())
        assert torch.equal(p3, prob)
        assert torch.equal(e3, ent) if want_ent else bool((e3 == -1).all())
        assert torch.equal(a3, area) if want_area else bool((a3 == -1).all())


# ------------------------------------------------------------------ argument contract
class _Calls:
    """Valid argument lists of both entry points, by name; an output filled with a sentinel that a refused call leaves."""

    def __init__(self):
        from al3d import detector_ops as D, lib
        from al3d.selector_ops import _ptr, _stream
        self.src = torch.randn(1, 5, 6, 8, device=DEV)
        tabs = D.bev_grid_tables([(-2.5, 2.5, 1.0), (-3.0, 3.0, 1.0)], [(-2.0, 2.0, 0.5), (-3.0, 3.0, 0.75)], (5, 6), DEV)
        self.H, self.W = tabs[0].shape[0], tabs[2].shape[0]
        self.out = torch.full((1, self.H, self.W, 8), -3.0, device=DEV)
        self.resample = dict(src=_ptr(self.src), N=1, h=5, w=6, C=8, row_idx=_ptr(tabs[0]), row_w=_ptr(tabs[1]),
                             col_idx=_ptr(tabs[2]), col_w=_ptr(tabs[3]), H=self.H, W=self.W, swapped=0, out=_ptr(self.out),
                             stream=_stream())
        self.tabs = tabs
        self.x = torch.randn(1, 4, 5, 8, device=DEV)
        self.wgt, self.b = torch.randn(3, 8, device=DEV), torch.randn(3, device=DEV)
        self.prob = torch.full((1, 3, 4, 5), -3.0, device=DEV)
        self.ent, self.area = torch.full((1, 3), -3.0, device=DEV), torch.full((1, 3), -3, dtype=torch.int32, device=DEV)
        self.ws = torch.empty(int(lib.load().al3d_seg_classify_workspace_bytes(1, 4, 5)), dtype=torch.uint8, device=DEV)
        self.classify = dict(x=_ptr(self.x), w=_ptr(self.wgt), b=_ptr(self.b), N=1, H=4, W=5, C=8, K=3, prob=_ptr(self.prob),
                             ent=_ptr(self.ent), area=_ptr(self.area), ws=_ptr(self.ws), stream=_stream())

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.out == -3.0).all() and (self.prob == -3.0).all() and (self.ent == -3.0).all() and (self.area == -3).all())


@pytest.fixture(scope="module")
def calls():
    return _Calls()


def _refused(calls, entry, fragment, **changed):
    from al3d import lib
    args = dict(calls.resample if entry == "al3d_bev_grid_resample_nhwc_f32" else calls.classify, **changed)
    with pytest.raises(lib.Al3dError) as err:
        lib.call(entry, *args.values())
    msg = str(err.value).split(": ", 1)[1]                # lib.check: "<entry> failed with status <n>: <library message>"
    assert msg.startswith(entry + ":") and fragment in msg, msg
    assert calls.untouched()                              # refused on the host: nothing was launched


RESAMPLE_REFUSALS = [("null pointer", dict(src=None)), ("null pointer", dict(col_w=None)), ("non-positive size", dict(N=0)),
                     ("non-positive size", dict(h=0)), ("non-positive size", dict(W=-1)), ("C=6 must be", dict(C=6)),
                     ("C=0 must be", dict(C=0)), ("out_hw_swapped=2", dict(swapped=2))]
CLASSIFY_REFUSALS = [("null pointer", dict(b=None)), ("null pointer", dict(prob=None)), ("non-positive size", dict(N=0)),
                     ("non-positive size", dict(W=0)), ("C=10 must be", dict(C=10)), ("K=0 is outside", dict(K=0)),
                     ("K=17 is outside", dict(K=17)), ("need a 4-byte aligned workspace", dict(ws=None)),
                     ("do not fit in LDS", dict(K=16, C=1024))]


@pytest.mark.parametrize("fragment,changed", RESAMPLE_REFUSALS)
def test_resample_refuses(calls, fragment, changed):
    _refused(calls, "al3d_bev_grid_resample_nhwc_f32", fragment, **changed)


@pytest.mark.parametrize("fragment,changed", CLASSIFY_REFUSALS)
def test_classify_refuses(calls, fragment, changed):
    _refused(calls, "al3d_seg_classify_f32", fragment, **changed)


def test_misaligned_bases_are_refused(calls):
    r, c = calls.resample, calls.classify
    _refused(calls, "al3d_bev_grid_resample_nhwc_f32", "16-byte aligned maps", src=r["src"] + 4)
    _refused(calls, "al3d_bev_grid_resample_nhwc_f32", "16-byte aligned maps", out=r["out"] + 8)
    _refused(calls, "al3d_bev_grid_resample_nhwc_f32", "8-byte aligned tables", row_w=r["row_w"] + 4)
    _refused(calls, "al3d_seg_classify_f32", "16-byte aligned map and weights", x=c["x"] + 4)
    _refused(calls, "al3d_seg_classify_f32", "16-byte aligned map and weights", w=c["w"] + 8)
    _refused(calls, "al3d_seg_classify_f32", "4-byte aligned bias and outputs", prob=c["prob"] + 2)


def test_valid_calls_run_and_a_wild_table_reads_nothing(calls):
    """The unchanged argument lists run (last, so that the sentinels above stay), and a table holding indices far outside
    the map gives zeros: the kernel checks every index against the map's size."""
    from al3d import lib
    from al3d.selector_ops import _ptr
    lib.call("al3d_bev_grid_resample_nhwc_f32", *calls.resample.values())
    lib.call("al3d_seg_classify_f32", *calls.classify.values())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(calls.out).all()) and float(calls.prob.min()) > 0 and float(calls.prob.max()) < 1
    wild = torch.tensor([[-7, 5]] * calls.H, dtype=torch.int32, device=DEV)
    lib.call("al3d_bev_grid_resample_nhwc_f32", *dict(calls.resample, row_idx=_ptr(wild)).values())
    torch.cuda.synchronize()
    assert bool((calls.out == 0).all())


# ------------------------------------------------------------------ module
def head_bounds(x, sd, i_s, o_s, C):
    """-> (float64 reference dict, elementwise bound of the probabilities): module docstring, 'Head'."""
    from dense_fp64 import E_MAX
    ref = Y.head64(x, sd, i_s, o_s)
    _, norm = Y.head_abs64(x, sd, i_s, o_s)
    return ref, 0.25 * (2.0 * E_MAX + 6.0 * Y.U + (C + 2) * Y.U) * norm + TIGHT_MAX["sigmoid"]


def golden_head(**kwargs):
    from al3d.models import build_head
    g = golden()
    head = build_head(dict(g["cfg"], type="BEVSegmentationHead", **kwargs))
    head.load_state_dict(g["sd"], strict=True)
    return head.to(DEV).eval()


def test_head_against_the_yardstick_and_the_golden():
    g = golden()
    i_s, o_s = scopes(g["cfg"])
    if "head" not in _REF:
        _REF["head"] = head_bounds(g["x"], g["sd"], i_s, o_s, 32)
    ref, bound = _REF["head"]
    head = golden_head()
    x = nhwc(g["x"]).to(DEV)
    with torch.no_grad():
        prob = head(x)
        prob_l, ent, area = head([x], with_stats=True)
    assert tuple(prob.shape) == (2, 6, 20, 23) and torch.equal(prob, prob_l)
    err = (prob.cpu().double() - ref["prob"]).abs()
    print(f"head: max err {float(err.max()):.3e}, max err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    gold = g["prob"].double()
    assert float((prob.cpu().double() - gold).abs().max() / gold.abs().max()) < 1e-5
    # the statistics are those of the returned probabilities
    assert torch.equal(area.cpu().long(), (prob.cpu() > 0.5).sum((-2, -1)))
    p = prob.cpu().double().clamp(1e-300, 1.0)
    q = (1.0 - prob.cpu().double()).clamp(1e-300, 1.0)
    mean_ent = -(p * p.log() + q * q.log()).mean((-2, -1))
    assert float((ent.cpu().double() - mean_ent).abs().max()) < 1e-5 and tuple(ent.shape) == (2, 6)
    # a map stored [y, x] with transpose_input=True: the same head, the same [B, K, X, Y] output
    with torch.no_grad():
        prob_t = golden_head(transpose_input=True)(x.permute(0, 2, 1, 3).contiguous())
    assert tuple(prob_t.shape) == (2, 6, 20, 23)
    err_t = (prob_t.cpu().double() - ref["prob"]).abs()
    print(f"head, transposed input: max err / bound {float((err_t / bound).max()):.3f}, "
          f"max difference from the plain head {float((prob_t - prob).abs().max()):.3e}")
    assert bool((err_t <= bound).all())


def test_other_arithmetics_in_a_child_process():
    """The head on the golden input under bf16x6 and f32 (AL3D_MATH is read at import): the same bound."""
    for math in ("bf16x6", "f32"):
        env = dict(os.environ, AL3D_MATH=math)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bev_seg_worker.py")], env=env, capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        out = json.loads(r.stdout.strip().splitlines()[-1])
        print(out)
        assert out["math"] == math and out["finite"] and out["shape"] == [2, 6, 20, 23] and out["err_over_bound"] <= 1.0
        assert out["golden"] < 1e-5


# ------------------------------------------------------------------ detector
def _camera_example(B, N, image_size):
    from test_camera_decoder_gpu import _rig
    K, c2l, img_aug, lidar_aug = _rig(B, N, image_size)
    return dict(img=torch.randn(B, N, *image_size, 3, generator=torch.Generator().manual_seed(12)).to(DEV),
                camera_intrinsics=K.to(DEV), camera2lidar=c2l.to(DEV), img_aug_matrix=img_aug.to(DEV),
                lidar_aug_matrix=lidar_aug.to(DEV), metadata=[dict(index=i) for i in range(B)])


def test_camera_only_detector_with_a_map_head():
    from al3d import synthetic
    from al3d.models import build_detector
    from test_camera_decoder_cpu import detector_cfg
    classes = ["drivable_area", "ped_crossing", "walkway", "stop_line", "carpark_area", "divider"]
    i_s, o_s = [(-6.4, 6.4, 0.8), (-3.2, 3.2, 0.8)], [(-5.0, 5.0, 0.5), (-3.0, 3.0, 0.5)]      # 16 x 8 cells -> 20 x 12
    map_head = dict(type="BEVSegmentationHead", in_channels=256, classes=classes, loss="focal",
                    grid_transform=dict(input_scope=i_s, output_scope=o_s))
    cfg = detector_cfg((64, 96), 32, None, grid_y=16)
    plain = build_detector(dict(cfg))
    det = build_detector(dict(cfg, map_head=map_head))
    # map_head=None: the module tree of the parent commit -- no key under heads.*; with it: the reference's heads.map.*
    plain_keys, keys = set(plain.state_dict()), set(det.state_dict())
    assert not any(k.startswith("heads.") for k in plain_keys) and plain.map_head is None and plain.bbox_head is None
    head_keys = {"heads.map." + k for k in build_detector(dict(cfg, map_head=map_head)).heads["map"].state_dict()}
    assert keys - plain_keys == head_keys and plain_keys <= keys and "heads.map.classifier.6.bias" in head_keys
    synthetic.seed_modules_(plain, 70)
    det.load_state_dict(plain.state_dict(), strict=False)             # the same encoders and decoder ...
    synthetic.seed_modules_(det.heads["map"], 71)                     # ... and a seeded head
    plain, det = plain.to(DEV).eval(), det.to(DEV).eval()
    ex = _camera_example(1, 2, (64, 96))
    with torch.no_grad():
        out_plain, mid_plain = plain(ex, return_loss=False, estimate=True)
        with pytest.raises(RuntimeError, match="without a bbox_head"):
            plain(ex, return_loss=False)
        out = det(ex, return_loss=False)                                   # no bbox_head, not estimate: works with a map head
        out_e, middle = det(ex, return_loss=False, estimate=True)
    assert out_plain == [dict(metadata=dict(index=0))]
    assert len(out) == 1 and set(out[0]) == {"metadata", "masks_bev", "map_entropy", "map_area"}
    assert tuple(out[0]["masks_bev"].shape) == (6, 20, 12) and tuple(out[0]["map_entropy"].shape) == (6,)
    assert tuple(out[0]["map_area"].shape) == (6,) and out[0]["map_area"].dtype == torch.int32
    assert torch.equal(out[0]["masks_bev"], out_e[0]["masks_bev"]) and out[0]["metadata"] == dict(index=0)
    # the decoder does not depend on the head: the same seeds give the same map, bit for bit
    dec = middle[-1].nhwc
    assert tuple(dec.shape) == (1, 16, 8, 256) and torch.equal(dec, mid_plain[-1].nhwc)
    sd = {k[len("heads.map."):]: v.cpu() for k, v in det.state_dict().items() if k.startswith("heads.map.")}
    ref, bound = head_bounds(dec.cpu().permute(0, 3, 1, 2), sd, i_s, o_s, 256)
    err = (out[0]["masks_bev"].cpu().double() - ref["prob"][0]).abs()
    print(f"detector map head: max err {float(err.max()):.3e}, max err / bound {float((err / bound[0]).max()):.3f}")
    assert bool((err <= bound[0]).all())
    assert torch.equal(out[0]["map_area"].cpu().long(), (out[0]["masks_bev"].cpu() > 0.5).sum((-2, -1)))
