#!/usr/bin/env python3
"""Generate the batch-preparation fixture g21_prep.npz by running the REFERENCE's own loaders.

Needs a checkout of chzhang18/RAG (``--reference DIR`` or the environment variable ``RAG_REFERENCE``); without one this script
exits with a message and changes nothing.  It writes small synthetic files (8-bit RGB PNGs, a 16-bit greyscale PNG, a PFM) and the
list files the loaders expect into a temporary directory, changes into it (src_self opens
``./filenames/drivingstereo/drivingstereo_cloudy_train.txt`` relative to the working directory), seeds ``random`` and calls

  * ``StereoDataset.__getitem__`` of ``src/dataloaders/stereo_dataset.py`` in training and evaluation mode (200x400 source),
  * ``SceneflowDrivingDataset.__getitem__`` of ``src_self/dataloaders/sceneflow_driving_dataset.py`` in both modes, and its
    ``transfer_color`` directly (odd 211x397 source, 150x230 real image).

Crop, pad, ``/ 256``, the PFM orientation and the colour transfer are therefore the reference's own code.  ONE step is not:
``torchvision`` is not installed where this runs, so ``data_io.get_transform`` gets a stand-in ``torchvision.transforms`` that
restates torchvision's arithmetic (``ToTensor``: HWC uint8 -> CHW, ``.to(float32).div(255)``; ``Normalize``:
``sub_(mean).div_(std)`` with float32 tensors of the mean and std).  That step is pinned by this definition, not by a run of
torchvision.  The four colour statistics are recomputed here with transfer_color's own two numpy expressions
(``x.mean(0).mean(0)``, ``x.std(0).std(0)`` of ``x = img.astype(float) / 255``), since the function does not return them.
One more shim: the loaders call ``np.lib.pad``, the alias of ``np.pad`` that numpy 2 dropped; it is restored as that alias.

The fixture stores the source arrays, the crop origins the reference drew (recovered by re-seeding ``random`` and repeating its
two ``randint`` calls; asserted against the ground-truth window it returned), the reference's outputs, and for the padded
evaluation outputs the un-padded window plus ``top_pad`` / ``right_pad`` (the rest is asserted to be zero here).  Content is
blocky-smooth (8x8 noise blocks, a horizontal ramp, a vertical staircase) so the fp32 outputs compress; no channel is constant.

Usage:  python tests/golden/make_golden_prep.py --reference /path/to/RAG
"""
import argparse
import os
import random
import sys
import tempfile
import types

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
CROP_H, CROP_W = 192, 384             # hard-coded upstream


def _torchvision_stand_in():
    class Compose:
        def __init__(self, transforms):
            self.transforms = transforms

        def __call__(self, x):
            for t in self.transforms:
                x = t(x)
            return x

    class ToTensor:
        def __call__(self, pic):
            a = np.array(pic, copy=True)
            assert a.dtype == np.uint8 and a.ndim == 3
            return torch.from_numpy(a).permute(2, 0, 1).contiguous().to(torch.float32).div(255)

    class Normalize:
        def __init__(self, mean, std):
            self.mean, self.std = mean, std

        def __call__(self, t):
            t = t.clone()
            mean = torch.as_tensor(self.mean, dtype=t.dtype)
            std = torch.as_tensor(self.std, dtype=t.dtype)
            return t.sub_(mean.view(-1, 1, 1)).div_(std.view(-1, 1, 1))

    tv, tr = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
    tr.Compose, tr.ToTensor, tr.Normalize = Compose, ToTensor, Normalize
    tv.transforms = tr
    sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tr


def _import_loader(tree, module, cls):
    """`cls` of dataloaders.<module> from one of the reference's trees (both name their package `dataloaders`)."""
    for k in [k for k in sys.modules if k == "dataloaders" or k.startswith("dataloaders.")]:
        del sys.modules[k]
    sys.path.insert(0, tree)
    try:
        mod = __import__(f"dataloaders.{module}", fromlist=[cls])
    finally:
        sys.path.remove(tree)
    return getattr(mod, cls)


def image(seed, H, W):
    r = np.random.RandomState(seed)
    blocks = np.kron(r.rand(H // 8 + 1, W // 8 + 1, 3), np.ones((8, 8, 1)))[:H, :W]
    ramp = np.linspace(0, 1, W)[None, :, None] * r.uniform(0.3, 1.0, 3)
    stair = (np.arange(H) // 4 * 4 / H)[:, None, None] * r.uniform(0.3, 1.0, 3)
    x = 0.45 * blocks + 0.35 * ramp + 0.2 * stair
    return np.clip(x * 255 * r.uniform(0.7, 1.05), 0, 255).astype(np.uint8)


def disparity(seed, H, W):
    r = np.random.RandomState(seed)
    blocks = np.kron(r.rand(H // 8 + 1, W // 8 + 1), np.ones((8, 8)))[:H, :W]
    d = 60.0 * blocks + 40.0 * np.linspace(0, 1, W)[None, :]
    d[blocks < 0.15] = 0.0                                   # holes, as in a sparse ground truth
    return d


def write_pfm(path, a):
    with open(path, "wb") as f:
        f.write(f"Pf\n{a.shape[1]} {a.shape[0]}\n-1.0\n".encode())
        np.flipud(a).astype("<f4").tofile(f)


def drawn_origin(seed, h, w):
    random.seed(seed)
    x1 = random.randint(0, w - CROP_W)
    y1 = random.randint(0, h - CROP_H)
    return np.array([y1, x1], dtype=np.int32)


def unpad(item, h, w, H, W):
    """The un-padded windows of an evaluation item; asserts the pad is what the reference says and zero."""
    top, right = int(item["top_pad"]), int(item["right_pad"])
    assert (top, right) == (H - h, W - w)
    out = {}
    for k in ("left", "right", "disparity"):
        a = np.asarray(item[k])
        assert a.shape[-2:] == (H, W) and a.dtype == np.float32
        assert not a[..., :top, :].any() and not a[..., :, w:].any(), "the pad is not zero"
        out[k] = np.ascontiguousarray(a[..., top:, :w])
    return out, top, right


def main():
    from PIL import Image
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("RAG_REFERENCE"))
    ref = ap.parse_args().reference
    if not ref or not os.path.isdir(os.path.join(ref, "src_self")):
        print("reference not present; golden fixtures are used as committed")
        return
    ref = os.path.abspath(ref)
    _torchvision_stand_in()
    if not hasattr(np.lib, "pad"):
        np.lib.pad = np.pad
    StereoDataset = _import_loader(os.path.join(ref, "src"), "stereo_dataset", "StereoDataset")
    SceneflowDrivingDataset = _import_loader(os.path.join(ref, "src_self"), "sceneflow_driving_dataset", "SceneflowDrivingDataset")

    arrays = {}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            # ---- src: 8-bit PNG views, 16-bit PNG disparity
            h, w = 200, 400
            left, right = image(1, h, w), image(2, h, w)
            gt16 = np.round(disparity(3, h, w) * 256).astype(np.uint16)
            Image.fromarray(left).save("a_left.png")
            Image.fromarray(right).save("a_right.png")
            Image.fromarray(gt16).save("a_disp.png")
            assert np.array_equal(np.array(Image.open("a_disp.png")), gt16) and np.array_equal(np.array(Image.open("a_left.png")), left)
            with open("a_list.txt", "w") as f:
                f.write("a_left.png a_right.png a_disp.png\n")
            arrays.update({"src::left_u8": left, "src::right_u8": right, "src::gt_u16": gt16})
            seed = 2101
            random.seed(seed)
            item = StereoDataset(0, ["a_list.txt"], True)[0]
            org = drawn_origin(seed, h, w)
            assert np.array_equal(item["disparity"], (gt16.astype(np.float32) / 256.)[org[0]:org[0] + CROP_H, org[1]:org[1] + CROP_W])
            arrays.update({"src::train::origin": org, "src::train::left": item["left"].numpy(), "src::train::right": item["right"].numpy(),
                           "src::train::gt": np.ascontiguousarray(item["disparity"])})
            win, top, rpad = unpad(StereoDataset(0, ["a_list.txt"], False)[0], h, w, 480, 960)
            arrays.update({"src::eval::left": win["left"], "src::eval::right": win["right"], "src::eval::gt": win["disparity"],
                           "src::eval::pad": np.array([top, rpad], dtype=np.int32), "src::eval::out_hw": np.array([480, 960], dtype=np.int32)})

            # ---- src_self: PFM disparity, colour transfer against a real image
            h, w = 211, 397
            left, right, real = image(4, h, w), image(5, h, w), image(6, 150, 230)
            gtf = disparity(7, h, w).astype(np.float32)
            Image.fromarray(left).save("b_left.png")
            Image.fromarray(right).save("b_right.png")
            Image.fromarray(real).save("b_real.png")
            write_pfm("b_disp.pfm", gtf)
            os.makedirs("filenames/drivingstereo")
            with open("filenames/drivingstereo/drivingstereo_cloudy_train.txt", "w") as f:
                f.write("b_real.png\n")
            with open("b_list.txt", "w") as f:
                f.write("b_left.png b_right.png b_disp.pfm\n")
            ds = SceneflowDrivingDataset(0, "b_list.txt", True)
            assert np.array_equal(ds.load_pfm_disp("b_disp.pfm"), gtf)
            arrays.update({"self::left_u8": left, "self::right_u8": right, "self::real_u8": real, "self::gt_f32": gtf})
            for name, a in (("left", left), ("right", right), ("real", real)):
                x = a.astype(float) / 255
                st = np.stack((x.mean(0).mean(0), x.std(0).std(0)), axis=-1)          # [3,2] float64
                assert st.dtype == np.float64 and (st[:, 1] > 1e-3).all()
                arrays[f"self::stats_{name}"] = st
            arrays["self::tc_left"] = ds.transfer_color(left, real)
            arrays["self::tc_right"] = ds.transfer_color(right, real)
            seed = 2102
            random.seed(seed)
            item = ds[0]
            org = drawn_origin(seed, h, w)
            assert np.array_equal(item["disparity"], gtf[org[0]:org[0] + CROP_H, org[1]:org[1] + CROP_W])
            arrays.update({"self::train::origin": org, "self::train::left": item["left"].numpy(), "self::train::right": item["right"].numpy(),
                           "self::train::gt": np.ascontiguousarray(item["disparity"])})
            win, top, rpad = unpad(SceneflowDrivingDataset(0, "b_list.txt", False)[0], h, w, 540, 960)
            arrays.update({"self::eval::left": win["left"], "self::eval::right": win["right"], "self::eval::gt": win["disparity"],
                           "self::eval::pad": np.array([top, rpad], dtype=np.int32), "self::eval::out_hw": np.array([540, 960], dtype=np.int32)})
        finally:
            os.chdir(cwd)

    for k, v in arrays.items():
        if "::train::" in k or "::eval::" in k:
            assert v.dtype in (np.float32, np.int32), (k, v.dtype)
    path = os.path.join(OUT, "g21_prep.npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    print(f"g21_prep.npz  {size / 1024:.1f} KiB")
    assert size < 1024 * 1024, "fixture over the 1 MiB limit"


if __name__ == "__main__":
    main()
