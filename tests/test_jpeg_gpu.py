"""GPU suite: the device half of the split JPEG decoder (csrc/jpeg.hip) == the installed Pillow's decode, byte for byte, and
the camera file loader fed JPEGs through it == the same loader decoding with Pillow."""
import ctypes
import io

import numpy as np
import pytest
import torch

from gen_golden_bevfusion_loading import synth_image
from test_jpeg_host import CASES, LAYOUTS, _encode, _pil, _scan_start, device_sizes, host_decode, stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def device_decode(items):
    """items: [(info, quant, coefs)] of ONE geometry -> [n, H, W, 3] uint8 through al3d_jpeg_idct_rgb_u8."""
    from al3d import lib
    from al3d.selector_ops import _ptr, _stream
    info = np.ascontiguousarray(items[0][0], dtype=np.int32)
    n = len(items)
    coefs = torch.from_numpy(np.stack([it[2] for it in items])).to(DEV)
    quant = torch.from_numpy(np.stack([it[1] for it in items]).view(np.int16)).to(DEV)
    ip = info.ctypes.data_as(ctypes.c_void_p)
    ws = torch.empty(max(int(lib.load().al3d_jpeg_workspace_bytes(ip, n)), 16), dtype=torch.uint8, device=DEV)
    out = torch.empty((n, int(info[1]), int(info[0]), 3), dtype=torch.uint8, device=DEV)
    lib.call("al3d_jpeg_idct_rgb_u8", _ptr(coefs), _ptr(quant), ip, n, _ptr(out), _ptr(ws), _stream())
    return out.cpu().numpy()


@pytest.mark.parametrize("case", range(len(CASES)))
def test_device_decode_equals_pillow(case):
    c = CASES[case]
    datas = [_encode(synth_image(10 + case, *c["hw"]), **c["kw"]),
             _encode(synth_image(90 + case, *c["hw"]), **dict(c["kw"], quality=min(95, c["kw"]["quality"] + 7)))]
    got = device_decode([host_decode(d) for d in datas])         # two images, two sets of quantisation tables, one launch
    for k, d in enumerate(datas):
        assert np.array_equal(got[k], _pil(d)), (case, k)


def test_device_decode_grayscale_and_extreme_content():
    from PIL import Image
    g = synth_image(3, 75, 101)[..., 0]
    buf = io.BytesIO()
    Image.fromarray(g).save(buf, format="JPEG", quality=80)
    assert np.array_equal(device_decode([host_decode(buf.getvalue())])[0], _pil(buf.getvalue()))
    rng = np.random.default_rng(2)
    hard = (rng.integers(0, 2, (64, 96, 3)) * 255).astype(np.uint8)          # saturated noise: clamps on every path
    hard[:, 48:] = np.array([255, 0, 255], np.uint8)
    for sub in (0, 1, 2):
        d = _encode(hard, quality=100, subsampling=sub)
        assert np.array_equal(device_decode([host_decode(d)])[0], _pil(d)), sub


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_device_decode_of_every_layout_equals_pillow(layout):
    """Every sampling layout the parser accepts, Pillow's encoder can write it or not (4:4:0 = the h1v2 branch, Cb and Cr with
    different factors, chroma at full resolution; streams of tests/jpeg_encode.py), at 61 x 83 and at the smallest frames that
    reach every branch of jp_upsample: H = 1, 2, 3, 4 under a vertical ratio of 2, W = 5, 6 (3 real chroma columns) under a
    horizontal one, W = 1 at 4:4:0.  Two pictures with different quantisation tables per launch; bytes equal to Pillow's."""
    differ = []
    for hw in device_sizes(layout):
        items = [stream(layout, hw, k) for k in (0, 1)]
        got = device_decode([host_decode(data) for data, _ in items])
        differ += [(hw, k) for k, (_, want) in enumerate(items) if not np.array_equal(got[k], want)]
    assert not differ


def _camera_pool(tmp_path, frames):
    """frames[s][k]: the bytes of sample s's camera k -> infos of an mmdet3d-format pool under tmp_path."""
    rng = np.random.default_rng(4)
    infos = []
    for s, cams_bytes in enumerate(frames):
        rng.normal(0, 10, (300, 5)).astype(np.float32).tofile(tmp_path / f"k{s}.bin")
        cams = {}
        for k, data in enumerate(cams_bytes):
            (tmp_path / f"s{s}_c{k}.jpg").write_bytes(data)
            cams[f"CAM_{k}"] = dict(data_path=f"s{s}_c{k}.jpg", sensor2lidar_rotation=np.eye(3),
                                    sensor2lidar_translation=np.zeros(3),
                                    camera_intrinsics=np.array([[300.0, 0, 200], [0, 300.0, 112], [0, 0, 1]]))
        infos.append(dict(token=f"t{s}", lidar_path=f"k{s}.bin", timestamp=1_000_000 * s, sweeps=[], cams=cams))
    return infos


def _camera_loader(infos, tmp_path, mode):
    from al3d.datasets import CameraLidarFileLoader
    vox = dict(range=[-54.0, -54.0, -5.0, 54.0, 54.0, 3.0], voxel_size=[0.075, 0.075, 0.2], max_points_in_voxel=10,
               max_voxel_num=120000)
    return CameraLidarFileLoader(infos, vox, None, batch_size=1, device=DEV, root=str(tmp_path), image_size=(64, 176),
                                 threads=2, decode_threads=2, jpeg=mode)


def test_camera_file_loader_frames_that_end_early(tmp_path):
    """A half-copied pool: on a truncated frame jpeg='split' raises what jpeg='pil' raises; a frame whose scan stops at an
    early EOI comes back with Pillow's pixels (the rest of the frame grey), its batch decoded but not split."""
    good = [_encode(synth_image(40 + k, 225, 400), quality=80) for k in range(4)]
    cut = good[3][:_scan_start(good[3]) + 2 * (len(good[3]) - _scan_start(good[3])) // 3]
    infos = _camera_pool(tmp_path, [good[:2], [good[2], cut], [good[2], cut + b"\xff\xd9"]])
    raised = {}
    for mode in ("pil", "split"):
        loader = _camera_loader(infos[:2], tmp_path, mode)
        with pytest.raises(Exception) as e:
            list(loader)
        raised[mode] = e.type
    assert raised["split"] is raised["pil"] and issubclass(raised["pil"], OSError)
    outs = {}
    for mode in ("pil", "split"):
        loader = _camera_loader([infos[0], infos[2]], tmp_path, mode)
        outs[mode] = [ex["img"].cpu().numpy() for ex in loader]
        assert loader.images_decoded == 4 and loader.images_split == (2 if mode == "split" else 0)
    for a, b in zip(outs["pil"], outs["split"]):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_camera_file_loader_waits_for_running_decode_jobs(tmp_path, monkeypatch):
    """A loader left after its first batch has decode jobs of the batches read ahead still running; they write through raw
    pointers into pinned buffers the next iteration reuses, so closing the iterator waits for them."""
    import threading
    import time
    from al3d.datasets import camera_files
    infos = _camera_pool(tmp_path, [[_encode(synth_image(50 + 2 * s + k, 225, 400), quality=80) for k in range(2)]
                                    for s in range(3)])
    want = [ex["img"].cpu().numpy() for ex in _camera_loader(infos, tmp_path, "pil")]
    lock, count, inner = threading.Lock(), dict(started=0, finished=0), camera_files._decode_jpeg_into

    def slow(*args):
        with lock:
            count["started"] += 1
        time.sleep(0.2)
        out = inner(*args)
        with lock:
            count["finished"] += 1
        return out

    monkeypatch.setattr(camera_files, "_decode_jpeg_into", slow)
    loader = _camera_loader(infos, tmp_path, "split")
    it = iter(loader)
    next(it)
    it.close()
    with lock:
        assert count["started"] == count["finished"] and 2 <= count["started"] <= 6, count
    got = [ex["img"].cpu().numpy() for ex in loader]
    assert loader.images_split == 2 + 6
    assert len(got) == len(want) and all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(got, want))


def test_camera_file_loader_split_jpeg_equals_pillow(tmp_path):
    """CameraLidarFileLoader on a pool whose camera frames are JPEGs: jpeg='split' (entropy decoding on host threads,
    the rest on the device) hands the detector the SAME normalised images, bit for bit, as jpeg='pil'; a batch holding
    a frame the split decoder does not take (progressive) is decoded by Pillow as a whole."""
    from PIL import Image
    from al3d.datasets import CameraLidarFileLoader
    rng = np.random.default_rng(4)
    infos = []
    for s in range(3):
        pts = rng.normal(0, 10, (300, 5)).astype(np.float32)
        pts.tofile(tmp_path / f"k{s}.bin")
        cams = {}
        for k, nm in enumerate(["CAM_FRONT", "CAM_BACK"]):
            Image.fromarray(synth_image(7 * s + k, 225, 400)).save(tmp_path / f"s{s}_{nm}.jpg", quality=80,
                                                                   progressive=(s == 2 and k == 1))
            cams[nm] = dict(data_path=f"s{s}_{nm}.jpg", sensor2lidar_rotation=np.eye(3), sensor2lidar_translation=np.zeros(3),
                            camera_intrinsics=np.array([[300.0, 0, 200], [0, 300.0, 112], [0, 0, 1]]))
        infos.append(dict(token=f"t{s}", lidar_path=f"k{s}.bin", timestamp=1_000_000 * s, sweeps=[], cams=cams))
    vox = dict(range=[-54.0, -54.0, -5.0, 54.0, 54.0, 3.0], voxel_size=[0.075, 0.075, 0.2], max_points_in_voxel=10,
               max_voxel_num=120000)
    outs = {}
    for mode in ("pil", "split"):
        loader = CameraLidarFileLoader(infos, vox, None, batch_size=1, device=DEV, root=str(tmp_path), image_size=(64, 176),
                                       threads=2, decode_threads=2, jpeg=mode)
        outs[mode] = [ex["img"].cpu().numpy() for ex in loader]
        if mode == "split":
            assert loader.images_split == 4 and loader.images_decoded == 6     # the third sample fell back as a whole
        else:
            assert loader.images_split == 0
    for a, b in zip(outs["pil"], outs["split"]):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
