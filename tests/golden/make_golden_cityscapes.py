#!/usr/bin/env python3
"""Generate the Cityscapes half-resolution fixture g22_cityscapes.npz by running the REFERENCE's own loader.

Needs a checkout of chzhang18/RAG (``--reference DIR`` or the environment variable ``RAG_REFERENCE``) and Pillow; without the
checkout this script exits with a message and changes nothing.  It writes a 24x1802 8-bit RGB pair and a 24x1802 16-bit disparity
PNG (wider than 1800, so the loader takes its Cityscapes branch; the content is make_golden_prep.py's blocky-smooth generators,
the disparity with zero holes) into a temporary directory, seeds ``random`` and calls ``StereoDataset.__getitem__`` of
``src_self/dataloaders/stereo_dataset.py`` in training mode: ``resize((1024, 512), Image.ANTIALIAS)`` of the three images (an
UPSCALE in y, a downscale in x), ``/ 256. / 2``, the 192x384 crop, ToTensor + Normalize.  The resize is Pillow's, the rest the
reference's own code, with make_golden_prep.py's three shims: the stand-in ``torchvision.transforms`` (torchvision is not installed
where this runs), ``np.lib.pad`` restored as the alias of ``np.pad`` that numpy 2 dropped, and here ``Image.ANTIALIAS`` restored
as the alias of ``Image.LANCZOS`` that Pillow 10 dropped (the same filter under its newer name).

The fixture stores the sources, the crop origin the reference drew (recovered by re-seeding ``random`` and repeating its two
``randint`` calls on the RESIZED size) and the reference's ``left``, ``right``, ``disparity``.  If the three fp32 outputs do not
fit under 1 MiB, rows [0:96] of each are kept (``rows`` says how many); the dropped rows are asserted here to equal
``rag_amd.data.prepare_batch_torch``'s, so no part of an output goes unchecked.

Usage:  python tests/golden/make_golden_cityscapes.py --reference /path/to/RAG
"""
import argparse
import os
import random
import sys
import tempfile

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from make_golden_prep import CROP_H, CROP_W, _import_loader, _torchvision_stand_in, disparity, drawn_origin, image  # noqa: E402

LIMIT = 1024 * 1024
KEEP_ROWS = 96


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
    if not hasattr(Image, "ANTIALIAS"):
        Image.ANTIALIAS = Image.LANCZOS
    StereoDataset = _import_loader(os.path.join(ref, "src_self"), "stereo_dataset", "StereoDataset")

    h, w, rh, rw = 24, 1802, 512, 1024
    left, right = image(11, h, w), image(12, h, w)
    gt16 = np.round(disparity(13, h, w) * 256).astype(np.uint16)
    assert (gt16 == 0).any() and (gt16 > 0).any()
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            Image.fromarray(left).save("c_left.png")
            Image.fromarray(right).save("c_right.png")
            Image.fromarray(gt16).save("c_disp.png")
            assert Image.open("c_disp.png").mode == "I;16" and np.array_equal(np.array(Image.open("c_disp.png")), gt16)
            with open("c_list.txt", "w") as f:
                f.write("c_left.png c_right.png c_disp.png\n")
            seed = 2201
            random.seed(seed)
            item = StereoDataset(0, ["c_list.txt"], True)[0]
        finally:
            os.chdir(cwd)
    org = drawn_origin(seed, rh, rw)                                 # the loader draws on the resized 1024x512 image
    ref_out = {"left": item["left"].numpy(), "right": item["right"].numpy(), "disparity": np.ascontiguousarray(item["disparity"])}
    for k, a in ref_out.items():
        assert a.dtype == np.float32 and a.shape[-2:] == (CROP_H, CROP_W), (k, a.dtype, a.shape)

    from rag_amd.data import CITYSCAPES_HALF, prepare_batch_torch
    t = lambda a: torch.from_numpy(a)[None]  # noqa: E731
    twin = prepare_batch_torch(t(left), t(right), t(gt16), out_hw=(CROP_H, CROP_W), origin=t(org), **CITYSCAPES_HALF)
    twin = {k: v[0].numpy() for k, v in zip(("left", "right", "disparity"), twin)}

    arrays = {"left_u8": left, "right_u8": right, "gt_u16": gt16, "origin": org}
    path = os.path.join(OUT, "g22_cityscapes.npz")
    for rows in (CROP_H, KEEP_ROWS):
        for k, a in ref_out.items():
            assert np.array_equal(a[..., rows:, :], twin[k][..., rows:, :]), f"dropped rows of {k} differ from prepare_batch_torch"
            arrays[k] = np.ascontiguousarray(a[..., :rows, :])
        arrays["rows"] = np.array(rows, dtype=np.int32)
        np.savez_compressed(path, **arrays)
        if os.path.getsize(path) < LIMIT:
            break
    size = os.path.getsize(path)
    print(f"g22_cityscapes.npz  {size / 1024:.1f} KiB, rows [0:{rows}] of each output; origin {org.tolist()}")
    assert size < LIMIT, "fixture over the 1 MiB limit"


if __name__ == "__main__":
    main()
