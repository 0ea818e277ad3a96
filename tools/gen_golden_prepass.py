"""Dev tool (needs the reference tree; not run by the tests).  Golden vectors for the PPAL / CALD pre-passes:
tests/golden/prepass_match.npz.

* The matching: the reference's OWN ``accumulate`` (classwise_weight_cald/algo.py:13-108, called class by class with
  ``dist_th = 1.0`` like classwise_weight_cald/evaluate.py:113-117) on synthetic frames.  The nuScenes devkit is not
  installed; the STAND-IN ``nuscenes.eval.*`` modules registered in its place hold only what algo.py imports (see
  ``STANDIN``).  The stand-in ``scale_iou`` also notes which two boxes it was called with -- accumulate calls it exactly
  once per match (algo.py:101) -- which is how the matched row of every prediction is known.
* The post-processing: ``main()`` of tools/ppal_unc.py and tools/cald_ent.py cannot run here (both build the dataset from
  a config and read / write files in the working directory; cald_ent.py:94 also writes to a hard-coded absolute path), so
  lines ppal_unc.py:69-98 and cald_ent.py:73-164 are RESTATED below with the same numpy / scipy / torch calls, as
  tests/selector_numpy.py does for the selectors.  They run on the synthetic frames' ``dict_p_iou`` and on a slice of 200
  frames of the reference's recorded tools/dict_p_iou.pkl (data its programs wrote), interleaved with frames that have no
  match.

Fixture conditions, enforced here (a prediction that breaks one is dropped before the reference runs; the rest are
asserted): no centre distance within 1e-4 of dist_th; sorted candidate distances of a prediction differ by more than 1e-4
unless they are exact ties of identical f32-representable coordinates; distinct per-frame consistency values are more
than 1e-4 apart; all coordinates and sizes are exactly representable in float32.  Only arrays and name lists are written.

  python tools/gen_golden_prepass.py
"""
import importlib
import os
import pickle
import sys

import numpy as np
import scipy.stats
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_import as RI  # noqa: E402

STANDIN = ("nuscenes.eval.common.data_classes.EvalBoxes -> a dict of sample_token -> box list with .all, .sample_tokens "
           "and [] (data_classes.py's container); nuscenes.eval.common.utils.center_distance = "
           "np.linalg.norm(pred.translation[:2] - gt.translation[:2]); scale_iou = prod(min(size_a, size_b)) / "
           "(prod(size_a) + prod(size_b) - that) for aligned boxes, plus a log of the (gt, pred) pair of every call; "
           "yaw_diff / velocity_l2 / attr_acc / cummean imported by algo.py but unused by accumulate: None; "
           "nuscenes.eval.detection.data_classes.DetectionMetricData: only no_predictions(), which the generator asserts is "
           "never reached (every class has a reference box); boxes: objects with sample_token, translation, size, "
           "detection_name, detection_score")
NAMES = ["car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian",
         "traffic_cone"]
DIST_TH = 1.0
B, NT, POST = 4, 3, 48
MATCHED = []            # (gt uid, pred uid) of every scale_iou call


class Box:
    def __init__(self, uid, token, xyz, size, name, score):
        self.uid, self.sample_token, self.translation, self.size = uid, token, tuple(xyz), tuple(size)
        self.detection_name, self.detection_score = name, score


class EvalBoxes:
    def __init__(self):
        self.boxes = {}

    def add_boxes(self, token, boxes):
        self.boxes.setdefault(token, []).extend(boxes)

    def __getitem__(self, token):
        return self.boxes[token]

    @property
    def sample_tokens(self):
        return list(self.boxes.keys())

    @property
    def all(self):
        return [b for t in self.sample_tokens for b in self.boxes[t]]


def center_distance(gt_box, pred_box):
    return np.linalg.norm(np.array(pred_box.translation[:2]) - np.array(gt_box.translation[:2]))


def scale_iou(sample_annotation, sample_result):
    MATCHED.append((sample_annotation.uid, sample_result.uid))
    sa_size, sr_size = np.array(sample_annotation.size), np.array(sample_result.size)
    assert all(sa_size > 0) and all(sr_size > 0)
    min_wlh = np.minimum(sa_size, sr_size)
    intersection = np.prod(min_wlh)
    union = np.prod(sa_size) + np.prod(sr_size) - intersection
    return intersection / union


class DetectionMetricData:
    @classmethod
    def no_predictions(cls):
        raise AssertionError("a class without reference boxes: the reference would return no dict here")


def import_accumulate():
    RI._mod("nuscenes")
    RI._mod("nuscenes.eval")
    RI._mod("nuscenes.eval.common")
    RI._mod("nuscenes.eval.detection")
    RI._mod("nuscenes.eval.common.data_classes", EvalBoxes=EvalBoxes)
    RI._mod("nuscenes.eval.common.utils", center_distance=center_distance, scale_iou=scale_iou, yaw_diff=None,
            velocity_l2=None, attr_acc=None, cummean=None)
    RI._mod("nuscenes.eval.detection.data_classes", DetectionMetricData=DetectionMetricData)
    sys.path.insert(0, RI.REFERENCE_ROOT)
    return importlib.import_module("classwise_weight_cald.algo").accumulate


def grid(rng, lo, hi, step, size=None):
    """Multiples of ``step`` (a power of two) in [lo, hi): exactly representable in float32."""
    return (rng.integers(int(lo / step), int(hi / step), size=size) * step).astype(np.float32)


def make_frames(rng):
    """Four frames of references and predictions on a 1/64 m grid: jittered copies of reference boxes (inside and outside
    the threshold), two predictions on one reference, references at exactly equal distances, equal scores, a near box of
    another class, false positives; frame 3 is dense."""
    boxes = np.zeros((B, NT, POST, 9), np.float32)
    scores = np.zeros((B, NT, POST), np.float32)
    labels = np.zeros((B, NT, POST), np.int32)
    counts = np.zeros((B, NT), np.int32)
    refs = []
    for b in range(B):
        nref = (24, 31, 17, 60)[b]
        rb = np.zeros((nref, 9), np.float32)
        rb[:, 0], rb[:, 1] = grid(rng, -40, 40, 1 / 64, nref), grid(rng, -40, 40, 1 / 64, nref)
        rb[:, 2] = grid(rng, -2, 1, 1 / 16, nref)
        rb[:, 3:6] = grid(rng, 0.5, 6, 1 / 16, (nref, 3))
        rl = rng.integers(0, 10, nref).astype(np.int32)
        rl[:10] = rng.permutation(10)                       # every class has a reference box in every frame
        rs = rng.uniform(0.05, 0.95, nref).astype(np.float32)
        # two references of one class at mirrored offsets from a prediction: an exact tie
        rb[1, :2] = rb[0, :2] + np.float32([1.0, 0.0])
        rl[1] = rl[0]
        cand = []                                           # (label, box9, score)
        tie = rb[0].copy()
        tie[0] += np.float32(0.5)                           # 0.5 from row 0 and from row 1
        cand.append((rl[0], tie, np.float32(0.625)))
        cand.append((rl[0], tie.copy(), np.float32(0.625)))           # same score: the later one goes first
        for r in range(2, nref):
            k = int(rng.integers(0, 4))
            for _ in range(k):
                p = rb[r].copy()
                far = rng.random() < 0.25
                p[:2] += grid(rng, 1.25, 3, 1 / 64, 2) * rng.choice([-1, 1], 2) if far else grid(rng, -0.625, 0.625, 1 / 64, 2)
                p[3:6] = np.maximum(np.float32(0.25), p[3:6] + grid(rng, -0.5, 0.5, 1 / 16, 3))
                lab = rl[r] if rng.random() < 0.85 else (rl[r] + 1) % 10      # a near box of another class
                sc = np.float32(rng.choice([0.25, 0.5, 0.75])) if rng.random() < 0.2 else np.float32(rng.uniform(0.1, 0.99))
                cand.append((lab, p, sc))
        for _ in range(6):                                  # false positives
            p = np.zeros(9, np.float32)
            p[:2], p[3:6] = grid(rng, -45, 45, 1 / 64, 2), grid(rng, 0.5, 6, 1 / 16, 3)
            cand.append((int(rng.integers(0, 10)), p, np.float32(rng.uniform(0.1, 0.99))))
        # fixture conditions per prediction
        kept = []
        for lab, p, sc in cand:
            d = np.sort(np.linalg.norm(rb[rl == lab, :2].astype(np.float64) - p[:2].astype(np.float64), axis=1))
            gaps = np.diff(d[d < 4.0])
            if np.any(np.abs(d - DIST_TH) <= 1e-4) or np.any((gaps != 0) & (gaps <= 1e-4)):
                continue
            kept.append((lab, p, sc))
        order = rng.permutation(len(kept))
        kept = [kept[i] for i in order][:NT * POST - 8]
        per = [len(kept) // NT + (1 if t < len(kept) % NT else 0) for t in range(NT)]
        at = 0
        for t in range(NT):
            for i in range(per[t]):
                lab, p, sc = kept[at]
                boxes[b, t, i], scores[b, t, i], labels[b, t, i] = p, sc, lab
                at += 1
            counts[b, t] = per[t]
            boxes[b, t, per[t]:, :] = 7.0                   # slots beyond the count hold junk that must not be read
            scores[b, t, per[t]:] = 0.99
            labels[b, t, per[t]:] = rl[2]
        refs.append((rb, rl, rs))
    return boxes, scores, labels, counts, refs


def run_reference(accumulate, boxes, scores, labels, counts, refs):
    gt, pred = EvalBoxes(), EvalBoxes()
    uid_pred, row0 = {}, 0
    ref_off = [0]
    for b in range(B):
        tok = f"frame{b}"
        rb, rl, rs = refs[b]
        gt.add_boxes(tok, [Box(row0 + r, tok, [float(v) for v in rb[r, :3]], [float(v) for v in rb[r, 3:6]], NAMES[rl[r]],
                               float(rs[r])) for r in range(len(rl))])
        row0 += len(rl)
        ref_off.append(row0)
        plist = []
        for t in range(NT):
            for i in range(counts[b, t]):
                uid = (b, t, i)
                plist.append(Box(uid, tok, [float(v) for v in boxes[b, t, i, :3]], [float(v) for v in boxes[b, t, i, 3:6]],
                                 NAMES[labels[b, t, i]], float(scores[b, t, i])))
        pred.add_boxes(tok, plist)
    dict_p_iou = {}
    for name in NAMES:
        dict_p_iou = accumulate(gt, pred, name, center_distance, DIST_TH, dict_p_iou)
        assert isinstance(dict_p_iou, dict)
    match_ref = np.full((B, NT, POST), -1, np.int32)
    match_iou = np.zeros((B, NT, POST), np.float64)
    for g, (b, t, i) in MATCHED:
        assert match_ref[b, t, i] == -1
        match_ref[b, t, i] = g
    # the iou of every match, in the order accumulate appended it per token and class
    seen = {}
    for g, (b, t, i) in MATCHED:
        tok = f"frame{b}"
        k = seen.get(tok, 0)
        match_iou[b, t, i] = dict_p_iou[tok]["iou"][k]
        assert dict_p_iou[tok]["detection_score"][k] == float(scores[b, t, i])
        seen[tok] = k + 1
    return dict_p_iou, match_ref, match_iou, np.asarray(ref_off, np.int32)


# ---- restated: ppal_unc.py:69-98 on a dict_p_iou and the labelled tokens
def ppal_weights(dict_p_iou_, selected_index_token):
    dict_p_iou_selected = [dict(dict_p_iou_[token_]) for token_ in selected_index_token if token_ in dict_p_iou_]
    for indx in range(len(dict_p_iou_selected)):
        dict_p_iou_selected[indx].update({'quality': []})
    for i in range(0, len(dict_p_iou_selected)):
        for j in range(0, len(dict_p_iou_selected[i]['name'])):
            quality = (dict_p_iou_selected[i]['detection_score'][j] ** 0.6) * (dict_p_iou_selected[i]['iou'][j] ** 0.4)
            dict_p_iou_selected[i]['quality'].append(quality)
    category_sum, category_count = {}, {}
    for i in range(len(dict_p_iou_selected)):
        for j in range(len(dict_p_iou_selected[i]['name'])):
            category = dict_p_iou_selected[i]['name'][j]
            quality = dict_p_iou_selected[i]['quality'][j]
            if category in category_sum:
                category_sum[category] += quality
                category_count[category] += 1
            else:
                category_sum[category] = quality
                category_count[category] = 1
    diff_category_average = {}
    class_weight_alpha = 3.
    class_weight_ub = 2.
    b = np.exp(1. / class_weight_alpha) - 1
    for category in category_sum:
        reverse_q = 1. - category_sum[category] / category_count[category]
        diff_category_average[category] = 1 + class_weight_alpha * np.log(b * reverse_q + 1) * class_weight_ub
    return diff_category_average


# ---- restated: cald_ent.py:73-164 on a dict_p_iou, all tokens in dataset order and the labelled indices
def cald_rankings(dict_p_iou_, tokens, selected_index):
    dict_p_iou_ = {k: {kk: list(vv) for kk, vv in v.items()} for k, v in dict_p_iou_.items()}
    pred_new = {t: {} for t in tokens}
    pred_keys = list(pred_new.keys())
    selected_index_token = [pred_keys[idx] for idx in selected_index]
    for key in pred_new.keys():
        pred_new[key].update({'consistency_img': 1.0})
    for key in dict_p_iou_.keys():
        dict_p_iou_[key].update({'consistency_img': 1.0})
    for key in dict_p_iou_.keys():
        for i in range(0, len(dict_p_iou_[key]['name'])):
            q = dict_p_iou_[key]['detection_score'][i]
            p = dict_p_iou_[key]['ref_score'][i]
            m = (p + q) / 2
            js = 0.5 * scipy.stats.entropy(p, m) + 0.5 * scipy.stats.entropy(q, m)
            if js < 0:
                js = 0
            dict_p_iou_[key]['consistency_img'] = min(dict_p_iou_[key]['consistency_img'], np.abs(
                dict_p_iou_[key]['iou'][i] + 0.5 * (1 - js) * (p + q) - 1.3).item())
            pred_new[key].update({'consistency_img': dict_p_iou_[key]['consistency_img']})
    sorted_indices = [index for index, _ in
                      sorted(enumerate(pred_new.keys()), key=lambda x: pred_new[x[1]]['consistency_img'])]
    dict_p_iou_selected = [dict_p_iou_[token_] for token_ in selected_index_token if token_ in dict_p_iou_]
    sorted_token_list = sorted(pred_new.keys(), key=lambda x: pred_new[x]['consistency_img'])
    sorted_idx_and_token = {}
    for i in range(len(sorted_indices)):
        sorted_idx_and_token[sorted_token_list[i]] = sorted_indices[i]
    sorted_res_, idx_list = {}, []
    for tk in sorted_token_list:
        if tk in dict_p_iou_.keys():
            sorted_res_.update({tk: dict_p_iou_[tk]})
            idx_list.append(sorted_idx_and_token[tk])
    category_sum, category_count = {}, {}
    for i in range(len(dict_p_iou_selected)):
        for j in range(len(dict_p_iou_selected[i]['name'])):
            category = dict_p_iou_selected[i]['name'][j]
            if category in category_sum:
                category_sum[category] += 0
                category_count[category] += 1
            else:
                category_sum[category] = 0
                category_count[category] = 1
    name_to_class = {value: key for key, value in enumerate(category_sum.keys())}
    for key in sorted_res_.keys():
        for i in range(len(sorted_res_[key]['name'])):
            sorted_res_[key]['name'][i] = name_to_class[sorted_res_[key]['name'][i]]
    img_cls = []
    for key in sorted_res_.keys():
        cls_corr = [0] * 10
        for i in range(len(sorted_res_[key]['name'])):
            cls_corr[sorted_res_[key]['name'][i]] += 1
        img_cls.append(cls_corr)
    category_count_new = {}
    for old_key, value in category_count.items():
        category_count_new[name_to_class[old_key]] = value
    num_labeled_samples = len(selected_index)
    num_classes = 10
    with torch.no_grad():
        result = []
        for i in range(num_labeled_samples):
            cls_corr = [0] * num_classes
            for cls, count in category_count_new.items():
                cls_corr[cls] = count
            result.append(cls_corr)
            _result = torch.tensor(np.mean(np.array(result), axis=0)).unsqueeze(0)
        p = torch.nn.functional.softmax(_result, -1)
        q = torch.nn.functional.softmax(torch.tensor((img_cls), dtype=torch.float64), -1)
        log_mean = ((p + q) / 2).log()
        KLDivLoss = nn.KLDivLoss(reduction='none')
        jsdiv = torch.sum(KLDivLoss(log_mean, p), dim=1) / 2 + torch.sum(KLDivLoss(log_mean, q), dim=1) / 2
        idx_to_jsdiv = {}
        for i in range(len(idx_list)):
            idx_to_jsdiv[idx_list[i]] = jsdiv[i].item()
    consistency = [pred_new[t]['consistency_img'] for t in tokens]
    return sorted_indices, idx_to_jsdiv, consistency


def recorded_slice(rng):
    """200 frames of the reference's recorded dict_p_iou.pkl as flat per-match arrays, spread over a pool of 260 frames
    (the other 60 have no match and stay at consistency 1.0)."""
    with open(os.path.join(RI.REFERENCE_ROOT, "tools", "dict_p_iou.pkl"), "rb") as f:
        rec = pickle.load(f)
    keys = list(rec.keys())[:200]
    n = 260
    slots = np.sort(rng.permutation(n)[:200])
    tokens = [f"empty{i}" for i in range(n)]
    d = {}
    for k, s in zip(keys, slots):
        tokens[s] = k
        d[k] = {kk: [float(v) if kk != "name" else v for v in vv] for kk, vv in rec[k].items()}
    frame, cls, score, iou, ref = [], [], [], [], []
    for i, t in enumerate(tokens):
        if t in d:
            for j, name in enumerate(d[t]["name"]):
                frame.append(i)
                cls.append(NAMES.index(name))
                score.append(d[t]["detection_score"][j])
                iou.append(d[t]["iou"][j])
                ref.append(d[t]["ref_score"][j])
    return d, tokens, dict(rec_frame=np.array(frame, np.int32), rec_cls=np.array(cls, np.int32),
                           rec_score=np.array(score, np.float64), rec_iou=np.array(iou, np.float64),
                           rec_ref_score=np.array(ref, np.float64), rec_num_frames=np.array(n))


def main():
    accumulate = import_accumulate()
    rng = np.random.default_rng(2024)
    boxes, scores, labels, counts, refs = make_frames(rng)
    dict_p_iou, match_ref, match_iou, ref_off = run_reference(accumulate, boxes, scores, labels, counts, refs)
    tokens = [f"frame{b}" for b in range(B)]
    # per (frame, class) reductions from the reference's own records, in its order
    cls_count = np.zeros((B, 10), np.int32)
    cls_quality = np.zeros((B, 10), np.float64)
    cls_cons = np.ones((B, 10), np.float64)
    for b, tok in enumerate(tokens):
        r = dict_p_iou[tok]
        for j, name in enumerate(r["name"]):
            c = NAMES.index(name)
            q, p = r["detection_score"][j], r["ref_score"][j]
            m = (p + q) / 2
            js = 0.5 * scipy.stats.entropy(p, m) + 0.5 * scipy.stats.entropy(q, m)
            assert js == 0
            cls_count[b, c] += 1
            cls_quality[b, c] += (q ** 0.6) * (r["iou"][j] ** 0.4)
            cls_cons[b, c] = min(cls_cons[b, c], np.abs(r["iou"][j] + 0.5 * (1 - js) * (p + q) - 1.3).item())
    frame_cons = np.minimum(1.0, cls_cons.min(axis=1))
    assert np.all(np.diff(np.sort(frame_cons)) > 1e-4), "per-frame consistency values too close"
    assert cls_count.sum() > 60 and (match_ref >= 0).sum() == cls_count.sum()
    # the restatement the GPU edge cases take their expected values from agrees with the reference's accumulate
    import prepass_numpy as PN
    ref_boxes = np.concatenate([r[0] for r in refs])
    ref_labels = np.concatenate([r[1] for r in refs])
    ref_scores = np.concatenate([r[2] for r in refs])
    mine = PN.match_frames(boxes, scores, labels, counts, ref_boxes, ref_labels, ref_scores, ref_off, 10, DIST_TH)
    assert np.array_equal(mine["match_ref"], match_ref) and np.array_equal(mine["cls_count"], cls_count)
    assert np.allclose(mine["match_iou"], match_iou, rtol=1e-15, atol=0)
    store = dict(standin=np.array(STANDIN), names=np.array(NAMES), dist_th=np.array(DIST_TH), boxes=boxes, scores=scores,
                 labels=labels, counts=counts, ref_boxes=ref_boxes, ref_labels=ref_labels, ref_scores=ref_scores,
                 ref_off=ref_off, match_ref=match_ref, match_iou=match_iou, cls_count=cls_count, cls_quality=cls_quality,
                 cls_cons=cls_cons)
    # post-processing on the synthetic frames (labelled: frames 0 and 2)
    w = ppal_weights(dict_p_iou, [tokens[i] for i in (0, 2)])
    store.update(syn_labelled=np.array([0, 2]), syn_weight_names=np.array(list(w.keys())),
                 syn_weight_vals=np.array(list(w.values()), np.float64))
    si, jd, _ = cald_rankings(dict_p_iou, tokens, [0, 1, 2, 3])
    store.update(syn_cald_labelled=np.array([0, 1, 2, 3]), syn_sorted=np.array(si), syn_jsdiv_keys=np.array(list(jd.keys())),
                 syn_jsdiv_vals=np.array(list(jd.values()), np.float64))
    # post-processing on the recorded slice
    d, rtokens, arrays = recorded_slice(rng)
    store.update(arrays)
    n = len(rtokens)
    lab_cald = {int(i) for i in rng.permutation(n)[:120]}
    for name in sorted({name for v in d.values() for name in v["name"]}):      # the reference raises KeyError otherwise
        lab_cald.add(next(i for i, t in enumerate(rtokens) if t in d and name in d[t]["name"]))
    lab_cald = sorted(lab_cald)
    seen = {name for i in lab_cald if rtokens[i] in d for name in d[rtokens[i]]["name"]}
    assert seen == {name for v in d.values() for name in v["name"]}, "a class matched outside the labelled set only"
    si, jd, cons = cald_rankings(d, rtokens, lab_cald)
    assert sum(1 for c in cons if c == 1.0) >= 60
    store.update(rec_cald_labelled=np.array(lab_cald), rec_sorted=np.array(si), rec_consistency=np.array(cons, np.float64),
                 rec_jsdiv_keys=np.array(list(jd.keys())), rec_jsdiv_vals=np.array(list(jd.values()), np.float64))
    # PPAL on a small labelled set that leaves at least one class without a match
    lab_ppal = [int(i) for i in rng.permutation(n)[:12]]
    w = ppal_weights(d, [rtokens[i] for i in lab_ppal])
    assert 0 < len(w) < 10, "the labelled set should leave a class absent"
    store.update(rec_ppal_labelled=np.array(lab_ppal), rec_weight_names=np.array(list(w.keys())),
                 rec_weight_vals=np.array(list(w.values()), np.float64))
    w = ppal_weights(d, [rtokens[i] for i in lab_cald])
    store.update(rec_weight_all_names=np.array(list(w.keys())), rec_weight_all_vals=np.array(list(w.values()), np.float64))
    out = os.path.join(ROOT, "tests", "golden", "prepass_match.npz")
    np.savez_compressed(out, **store)
    print("wrote", out, os.path.getsize(out), "bytes;", int(cls_count.sum()), "matches of", int(counts.sum()),
          "predictions;", len(arrays["rec_frame"]), "recorded matches")


if __name__ == "__main__":
    main()
