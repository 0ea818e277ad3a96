#!/usr/bin/env python3
"""The PPAL / CALD pre-passes from a checkpoint and an infos file alone (al3d/selectors/prepass.py): the files
``PPALSelector`` (``class_weight_file``) and ``CaldSelector`` (``buffer_path``, ``jsdiv_path``) replay.

    python tools/active_prepass.py --config examples/active/cbgs_ppal.py --checkpoint latest.pth --mode ppal \\
        --out tools/diff_category_average.json
    python tools/active_prepass.py --config examples/active/cbgs_cald.py --checkpoint latest.pth --mode cald \\
        --view 1 0 0.0 1.0 --out data/buffers/cald_ent_sorted_idx.json --jsdiv idx_to_jsdiv.pkl
    python tools/active_prepass.py --config examples/active/estimator/cbgs_partial.py --checkpoint latest.pth \\
        --iou-targets work_dirs/iou_targets.npz
    torchrun --nproc-per-node 8 tools/active_prepass.py ...                 # every rank sweeps a contiguous shard

``ppal`` replaces the reference's tools/ppal_pred_list.py + tools/ppal_unc.py: one sweep, the detections matched to the
``gt_boxes`` / ``gt_names`` of ``cfg.selector.infos_origin`` (``ref_scores`` = -1.0), class weights from the labelled
frames.  ``cald`` replaces tools/cald_pred_list.py + tools/cald_ent.py: a plain sweep whose detections are the reference
boxes, a second sweep over the augmented ``--view`` (flip_x flip_y rot scale) matched against them.  The labelled frames
are the last round of ``cfg.selector.buffer_file``.  ``--iou-targets`` writes what the reference's Estimator is trained
against (det3d/models/detectors/estimator.py:98-115): ``off [N+1]`` and per detection ``best_iou`` (3-D IoU with the best
ground-truth box of ``infos_origin``), ``best_ref``, ``scores``, ``labels`` -- for every detection, where the reference
keeps only the boxes that contain a point (estimator.py:491).  The pool and the loaders are those of tools/active_select.py
(``--synthetic-scenes`` generates a pool; otherwise the infos' sweep files are read from ``cfg.data_root``).
"""
import argparse
import logging
import os
import pickle
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def parse_args():
    p = argparse.ArgumentParser(description="PPAL / CALD pre-pass")
    p.add_argument("--config", required=True)
    p.add_argument("--checkpoint", default=None)
    p.add_argument("--mode", choices=["ppal", "cald"], default=None)
    p.add_argument("--iou-targets", default=None, metavar="OUT.npz",
                   help="write the Estimator's training targets: every detection's best IoU against the ground truth")
    p.add_argument("--iou-metric", default="iou3d")
    p.add_argument("--iou-same-class", action="store_true")
    p.add_argument("--out", default=None, help="ppal: class_weight_file; cald: buffer_path (default: the selector's own)")
    p.add_argument("--jsdiv", default=None, help="cald: jsdiv_path (.pkl or .json)")
    p.add_argument("--view", nargs=4, type=float, default=[1, 0, 0.0, 1.0], metavar=("FLIP_X", "FLIP_Y", "ROT", "SCALE"))
    p.add_argument("--range-filter", action="store_true",
                   help="ppal: the devkit's class_range rule (detection_cvpr_2019), measured from the ego origin")
    p.add_argument("--local_rank", type=int, default=0)
    p.add_argument("--synthetic-scenes", type=int, default=0)
    p.add_argument("--batch", type=int, default=8)
    return p.parse_args()


def main():
    args = parse_args()
    if args.mode is None and args.iou_targets is None:
        raise SystemExit("active_prepass: give --mode ppal | cald and / or --iou-targets OUT.npz")
    from al3d import synthetic
    from al3d.datasets import DeviceSweepLoader, FileSweepLoader, PoolFrames, generate_task_anchors
    from al3d.models import build_detector
    from al3d.models.readers import needs_point_slots
    from al3d.selectors import prepass as P
    from al3d.utils import Config, fileio

    cfg = Config.fromfile(args.config)
    local_rank = int(os.environ.get("LOCAL_RANK", args.local_rank))
    distributed = int(os.environ.get("WORLD_SIZE", "1")) > 1
    if distributed:
        torch.cuda.set_device(local_rank)
        torch.distributed.init_process_group(backend=os.environ.get("AL3D_DIST_BACKEND", "nccl"), init_method="env://")
    rank = torch.distributed.get_rank() if distributed else 0
    world = torch.distributed.get_world_size() if distributed else 1
    logging.basicConfig(level=logging.INFO if rank == 0 else logging.ERROR)
    logger = logging.getLogger("active_prepass")
    sel_cfg = cfg.selector
    if args.synthetic_scenes:
        infos, _ = synthetic.make_pool(args.synthetic_scenes, seed=0)
        if rank == 0:
            os.makedirs(os.path.dirname(sel_cfg.infos_origin) or ".", exist_ok=True)
            with open(sel_cfg.infos_origin, "wb") as f:
                pickle.dump(infos, f)
    else:
        infos = fileio.load(sel_cfg.infos_origin)
    buffer = fileio.load(sel_cfg.buffer_file)
    labelled = list(buffer[str(max(int(k) for k in buffer))])

    dev = torch.device("cuda", local_rank)
    model = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    if args.checkpoint:
        sd = torch.load(args.checkpoint, map_location="cpu", weights_only=True)
        sd = sd.get("state_dict", sd)
        model.load_state_dict({k[7:] if k.startswith("module.") else k: v for k, v in sd.items()}, strict=False)
    else:
        synthetic.seeded_init_(model, seed=0)
    model = model.to(dev).eval()
    n = len(infos)
    per = (n + world - 1) // world
    mine = list(range(rank * per, min(n, (rank + 1) * per)))
    head_cfg = cfg.model.get("bbox_head")
    anchors = generate_task_anchors(cfg.tasks, cfg.target_assigner.anchor_generators, [1, 128, 128]) \
        if head_cfg is not None and head_cfg.get("type") == "MultiGroupHead" else None
    with_points = needs_point_slots(cfg.model.get("reader"))
    # DynamicPillarFeatureNet pools over the batch's points by point2voxel: no padded slots, the points themselves
    keep_points = cfg.model.get("reader", {}).get("type") == "DynamicPillarFeatureNet"
    if args.synthetic_scenes:
        pool = PoolFrames.from_synthetic(len(mine), dev, seed=1000 + rank)
        loader = DeviceSweepLoader(pool, cfg.voxel_generator, anchors, batch_size=args.batch, device=dev,
                                   with_points=with_points, keep_points=keep_points)
    else:
        loader = FileSweepLoader([infos[i] for i in mine], cfg.voxel_generator, anchors, batch_size=args.batch, device=dev,
                                 nsweeps=cfg.nsweeps, root=cfg.data_root,
                                 threads=int(os.environ.get("AL3D_READER_THREADS", "8")), with_points=with_points)
    loader.sampler = mine

    if args.iou_targets:
        t = P.run_iou_targets(model, loader, dev, infos, args.iou_targets, metric=args.iou_metric,
                              same_class=args.iou_same_class)
        logger.info("IoU targets of %d detections in %d frames -> %s", len(t["best_iou"]), n, args.iou_targets)
    if args.mode == "ppal":
        out = args.out or sel_cfg.get("class_weight_file", "tools/diff_category_average.json")
        weights = P.run_ppal_prepass(model, loader, dev, infos, labelled, out, range_filter=args.range_filter)
        logger.info("class weights of %d labelled frames -> %s: %s", len(labelled), out, weights)
    elif args.mode == "cald":
        out = args.out or sel_cfg.get("buffer_path", "cald_ent_sorted_idx.json")
        jsdiv = args.jsdiv or sel_cfg.get("jsdiv_path", "idx_to_jsdiv.pkl")
        view = (bool(args.view[0]), bool(args.view[1]), float(args.view[2]), float(args.view[3]))
        ranking, table = P.run_cald_prepass(model, loader, dev, n, labelled, view, out, jsdiv)
        logger.info("consistency ranking of %d frames -> %s; divergence of %d frames -> %s", len(ranking), out,
                    len(table), jsdiv)


if __name__ == "__main__":
    main()
