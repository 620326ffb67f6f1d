"""evaluation/eval_image_folder.py on the HIP kernels: PSNR, SSIM and LPIPS of a folder of renders against a folder
of ground-truth images, without skimage, imageio, lpips or torchvision.  The metrics come from iron_amd.image_metrics.

    python -m iron_amd.eval_image_folder FOLDER1 FOLDER2 [--alexnet ALEXNET.pth --lpips-lin ALEX_LIN.pth]

For every `*.jpg` of FOLDER1 and the `.png` of the same stem (`name.split('.')[0]`) in FOLDER2 one line of FOLDER1/../metrics.txt,
then the averages, in the reference's layout.  Deliberate deviations from the reference script:
  * names are processed in sorted order (the reference's `glob` order is the file system's);
  * an image that is not 8-bit RGB, a missing partner or a size mismatch raises IronError naming the file (the reference fails
    somewhere inside numpy or skimage);
  * the LPIPS weights are arguments: torchvision's AlexNet checkpoint and the lpips package's weights/v0.1/alex.pth, read from
    disk, never downloaded.  Without them PSNR and SSIM are computed, the LPIPS column holds `nan` and stderr says so.
"""
from __future__ import annotations

import argparse
import glob
import os
import sys

import numpy as np

from ._lib import IronError
from .image_metrics import LPIPS, evaluate_pair, format_metrics  # noqa: F401  (format_metrics, evaluate_pair: this module's API too)


def read_image_u8(fpath) -> np.ndarray:
    """An 8-bit RGB file as uint8 [H, W, 3] (the reference's imageio.imread before its `/ 255.`)."""
    from PIL import Image
    if not os.path.exists(fpath):
        raise IronError("eval_image_folder: %s does not exist" % fpath)
    with Image.open(fpath) as im:
        if im.mode != "RGB":
            raise IronError("eval_image_folder: %s is not an 8-bit RGB image (PIL mode %s)" % (fpath, im.mode))
        a = np.asarray(im, dtype=np.uint8)
    return np.ascontiguousarray(a)


def image_pairs(folder1, folder2):
    """[(name, jpg path in folder1, png path in folder2)] in sorted order of the names."""
    out = []
    for fpath in sorted(glob.glob(os.path.join(folder1, '*.jpg'))):
        name = os.path.basename(fpath)
        out.append((name, fpath, os.path.join(folder2, name.split('.')[0] + '.png')))
    return out


def eval_image_folder(folder1, folder2, lpips=None):
    """Scores every pair, writes folder1/../metrics.txt and returns the rows [(name, psnr, ssim, lpips)]."""
    rows = []
    for name, p1, p2 in image_pairs(folder1, folder2):
        pred_im = read_image_u8(p1)
        if not os.path.exists(p2):
            raise IronError("eval_image_folder: %s has no partner %s" % (p1, p2))
        trgt_im = read_image_u8(p2)
        if pred_im.shape != trgt_im.shape:
            raise IronError("eval_image_folder: %s is %d x %d but %s is %d x %d" % (p1, pred_im.shape[1], pred_im.shape[0], p2,
                                                                                  trgt_im.shape[1], trgt_im.shape[0]))
        rows.append((name,) + tuple(evaluate_pair(pred_im, trgt_im, lpips=lpips)))
    with open(os.path.join(folder1, '../metrics.txt'), 'w+') as fp:
        fp.write(format_metrics(rows))
    return rows


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(prog="python -m iron_amd.eval_image_folder", description=__doc__.split("\n\n")[0])
    ap.add_argument("folder1", help="renders (*.jpg); metrics.txt is written next to this folder")
    ap.add_argument("folder2", help="ground truth (the .png of the same stem)")
    ap.add_argument("--alexnet", help="torchvision's AlexNet checkpoint (features.{0,3,6,8,10}.{weight,bias})")
    ap.add_argument("--lpips-lin", help="the lpips package's weights/v0.1/alex.pth (lin{0..4}.model.1.weight)")
    args = ap.parse_args(sys.argv[1:] if argv is None else argv)
    if bool(args.alexnet) != bool(args.lpips_lin):
        raise SystemExit("eval_image_folder: --alexnet and --lpips-lin go together")
    try:
        lpips = None
        if args.alexnet:
            lpips = LPIPS.from_files(args.alexnet, args.lpips_lin)
        else:
            print("eval_image_folder: no LPIPS weights given (--alexnet, --lpips-lin): the lpips column is nan", file=sys.stderr)
        eval_image_folder(args.folder1, args.folder2, lpips=lpips)
    except IronError as e:
        raise SystemExit("error: %s" % e)


if __name__ == "__main__":
    main()
