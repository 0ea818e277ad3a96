#!/usr/bin/env python3
"""The data-preparation step of an active-learning round (reference tools/create_data.py:21-37):

    python tools/create_data.py nuscenes_data_prep --root_path data/nuScenes --version v1.0-trainval \\
        --nsweeps 10 --suffix 600

reads ``<root_path>/infos_train_10sweeps_withvelo_600.pkl`` (what ``tools/active_select.py`` dumped for the round; or
``--info_path``) and writes ``<root_path>/gt_database_10sweeps_withvelo_600/*.bin`` and
``<root_path>/dbinfos_train_10sweeps_withvelo_600.pkl`` (``al3d.datasets.create_groundtruth_database``).

Without ``--suffix`` the reference first builds the infos of the whole split with the nuScenes devkit
(``create_nuscenes_infos``); that half is not built here, so the command refuses unless ``--info_path`` names infos that
exist already.  ``--lidar_root`` is joined in front of relative ``lidar_path`` entries (the reference opens them as they
are, relative to the working directory)."""
import argparse
import os
import sys
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def nuscenes_data_prep(root_path, version, nsweeps=10, suffix=None, info_path=None, **kwargs):
    if suffix is None and info_path is None:
        raise SystemExit("create_data.py nuscenes_data_prep: without --suffix the reference builds the infos of the whole "
                         f"split ({version}) with the nuScenes devkit first; building infos needs the devkit and is not "
                         "built here.  Pass --suffix S (reads infos_train_<nsweeps>sweeps_withvelo_S.pkl, the file "
                         "tools/active_select.py dumps for a round) or --info_path P.")
    from al3d.datasets.create_gt_database import create_groundtruth_database
    if info_path is None:
        info_path = Path(root_path) / f"infos_train_{nsweeps:02d}sweeps_withvelo_{suffix}.pkl"
    extra = {k: v for k, v in kwargs.items() if v is not None}
    if suffix is not None:
        extra["suffix"] = suffix
    return create_groundtruth_database("NUSC", root_path, info_path, nsweeps=nsweeps, **extra)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="command", required=True)
    p = sub.add_parser("nuscenes_data_prep", help="ground-truth database of the infos of one round")
    p.add_argument("--root_path", required=True)
    p.add_argument("--version", required=True)
    p.add_argument("--nsweeps", type=int, default=10)
    p.add_argument("--suffix", default=None)
    p.add_argument("--info_path", default=None)
    p.add_argument("--lidar_root", default=None, help="directory in front of relative lidar_path entries")
    p.add_argument("--batch_size", type=int, default=None, help="frames per batch (default 4)")
    a = ap.parse_args(argv)
    nuscenes_data_prep(a.root_path, a.version, nsweeps=a.nsweeps, suffix=a.suffix, info_path=a.info_path,
                       lidar_root=a.lidar_root, batch_size=a.batch_size)


if __name__ == "__main__":
    main()
