"""Lat-long environment maps for the environment render of an exported asset (csrc/envlight.hip): the map
with its sampling distribution on the GPU, and the readers of the files a light probe comes in.

Convention (include/iron_hip.h, iron_mesh_occluded block): Mitsuba 0.6's `envmap` emitter, which the reference's
rgb_envmap_hdr_mat.xml uses: a world direction d, taken to the map's frame by to_world^T, has u = atan2(d.x, -d.z) / 2 pi wrapped to
[0, 1) and v = acos(d.y) / pi; the texel is (floor(v He), floor(u We)), clamped.  Radiance is constant per texel (Mitsuba
interpolates); the convention is not pinned to a Mitsuba render.  There is no CPU path: CPU tensors are refused.
"""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import torch

from . import _args, _lib

WHAT = "environment map"  # what this module's messages begin with


class EnvMap:
    """image [He, We, 3] linear radiance (numpy or a CUDA tensor; finite and >= 0, else IronError), to_world an optional 3x3
    rotation (the identity is the reference scene's default).  Builds the sampling distribution once, on the device: texel weight
    (0.2126 R + 0.7152 G + 0.0722 B) sin(pi (row + 1/2) / He), fp64 row CDFs and the marginal CDF.  Waits once (the check)."""

    def __init__(self, image, to_world=None, device=None):
        dev = torch.device(device) if device is not None else _args.pick_device(WHAT, image)
        _args.refuse_cpu(WHAT, image, to_world)
        if dev.type != "cuda":
            raise _lib.IronError("EnvMap: the device must be a GPU, got %s" % dev)
        img = _args.as_tensor(image, WHAT)
        if img.dim() != 3 or img.shape[2] != 3 or img.shape[0] * img.shape[1] == 0 or img.shape[0] * img.shape[1] > 1 << 24:
            raise _lib.IronError("EnvMap: image must be [He, We, 3] with 0 < He * We <= 2^24, got %s" % (tuple(img.shape),))
        R = np.eye(3) if to_world is None else np.asarray(to_world.detach().cpu() if isinstance(to_world, torch.Tensor) else to_world,
                                                          dtype=np.float64)
        if R.shape != (3, 3) or not np.isfinite(R).all() or np.abs(R @ R.T - np.eye(3)).max() > 1e-4:
            raise _lib.IronError("EnvMap: to_world must be a 3x3 rotation")
        self.device = dev
        self.to_world = R.astype(np.float32)
        with torch.cuda.device(dev):
            self.image = img.to(device=dev, dtype=torch.float32).contiguous()
            if not bool((torch.isfinite(self.image) & (self.image >= 0)).all()):
                raise _lib.IronError("EnvMap: radiance must be finite and >= 0")
            self.height, self.width = int(self.image.shape[0]), int(self.image.shape[1])
            lib = _lib.load()
            self.dist = _args.sized_workspace(lib.iron_envmap_workspace_bytes, self.height, self.width, device=dev)
            _lib.check(lib.iron_envmap_build(self.image.data_ptr(), self.height, self.width, self.dist.data_ptr(), _lib.stream_ptr(dev)))

    def c_struct(self) -> _lib.iron_envmap:
        return _lib.iron_envmap(self.image.data_ptr(), self.dist.data_ptr(), self.height, self.width,
                                (C.c_float * 9)(*[float(x) for x in self.to_world.reshape(-1)]))

    def _dirs(self, dirs):
        return _args.device_array(dirs, torch.float32, self.device, "dir", (3,), what=WHAT)

    def sample(self, u):
        """u [n, 2] in (0, 1) -> (texel int32 [n, 2] (row, col), dir fp32 [n, 3] world, pdf fp32 [n]): u[:, 0] picks the column,
        u[:, 1] the row; pdf = P(texel) We He / (2 pi^2 sin theta(dir)), the solid-angle density.  A texel of weight 0 is never
        returned; an all-black map gives pdf 0."""
        with torch.cuda.device(self.device):
            uu = _args.device_array(u, torch.float32, self.device, "u", (2,), what=WHAT)
            n = int(uu.shape[0])
            texel = torch.empty((n, 2), dtype=torch.int32, device=self.device)
            d = torch.empty((n, 3), dtype=torch.float32, device=self.device)
            pdf = torch.empty((n,), dtype=torch.float32, device=self.device)
            env = self.c_struct()
            _lib.check(_lib.load().iron_envmap_sample(C.byref(env), uu.data_ptr(), n, texel.data_ptr(), d.data_ptr(), pdf.data_ptr(),
                                                      _lib.stream_ptr(self.device)))
        return texel, d, pdf

    def pdf(self, dirs):
        """dirs [n, 3] world -> the solid-angle density of `sample` there, fp32 [n] (0 in a texel of weight 0)."""
        with torch.cuda.device(self.device):
            d = self._dirs(dirs)
            out = torch.empty((d.shape[0],), dtype=torch.float32, device=self.device)
            env = self.c_struct()
            _lib.check(_lib.load().iron_envmap_pdf(C.byref(env), d.data_ptr(), d.shape[0], out.data_ptr(), _lib.stream_ptr(self.device)))
        return out

    def lookup(self, dirs):
        """dirs [n, 3] world -> the radiance there, fp32 [n, 3]."""
        with torch.cuda.device(self.device):
            d = self._dirs(dirs)
            out = torch.empty((d.shape[0], 3), dtype=torch.float32, device=self.device)
            env = self.c_struct()
            _lib.check(_lib.load().iron_envmap_lookup(C.byref(env), d.data_ptr(), d.shape[0], out.data_ptr(), _lib.stream_ptr(self.device)))
        return out


# ---- files ----
def read_hdr(path) -> np.ndarray:
    """A Radiance .hdr picture (RGBE; flat or new-style run-length encoded scanlines, '-Y H +X W' orientation) -> float32
    [H, W, 3]: channel = mantissa 2^(exponent - 136), 0 where the exponent byte is 0."""
    with open(path, "rb") as fp:
        data = fp.read()
    if not (data.startswith(b"#?RADIANCE") or data.startswith(b"#?RGBE")):
        raise _lib.IronError("%s is not a Radiance picture" % path)
    end = data.find(b"\n\n")
    if end < 0:
        raise _lib.IronError("%s: no end of header" % path)
    if b"FORMAT=32-bit_rle_xyze" in data[:end]:
        raise _lib.IronError("%s: XYZE pictures are not supported" % path)
    eol = data.find(b"\n", end + 2)
    m = re.fullmatch(rb"-Y (\d+) \+X (\d+)", data[end + 2:eol].strip())
    if not m:
        raise _lib.IronError("%s: only the '-Y H +X W' orientation is supported" % path)
    H, W = int(m.group(1)), int(m.group(2))
    buf = np.frombuffer(data, dtype=np.uint8, offset=eol + 1)
    rgbe = np.empty((H, W, 4), dtype=np.uint8)
    pos = 0
    for y in range(H):
        if 8 <= W < 32768 and pos + 4 <= buf.size and buf[pos] == 2 and buf[pos + 1] == 2 and (int(buf[pos + 2]) << 8 | int(buf[pos + 3])) == W:
            pos += 4
            for ch in range(4):
                x = 0
                while x < W:
                    if pos >= buf.size:
                        raise _lib.IronError("%s: truncated scanline %d" % (path, y))
                    cnt = int(buf[pos])
                    if cnt > 128:
                        cnt -= 128
                        if cnt == 0 or x + cnt > W or pos + 2 > buf.size:
                            raise _lib.IronError("%s: bad run in scanline %d" % (path, y))
                        rgbe[y, x:x + cnt, ch] = buf[pos + 1]
                        pos += 2
                    else:
                        if cnt == 0 or x + cnt > W or pos + 1 + cnt > buf.size:
                            raise _lib.IronError("%s: bad run in scanline %d" % (path, y))
                        rgbe[y, x:x + cnt, ch] = buf[pos + 1:pos + 1 + cnt]
                        pos += 1 + cnt
                    x += cnt
        else:  # a flat scanline
            if pos + 4 * W > buf.size:
                raise _lib.IronError("%s: truncated scanline %d" % (path, y))
            rgbe[y] = buf[pos:pos + 4 * W].reshape(W, 4)
            pos += 4 * W
    e = rgbe[..., 3].astype(np.int32)
    scale = np.where(e > 0, np.ldexp(1.0, e - 136), 0.0)
    return (rgbe[..., :3].astype(np.float64) * scale[..., None]).astype(np.float32)


def read_envmap(path) -> np.ndarray:
    """.npy, Radiance .hdr (read_hdr), or .exr through imageio when it has an EXR plugin -> float32 [He, We, 3]."""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npy":
        img = np.load(path, allow_pickle=False)
    elif ext == ".hdr":
        img = read_hdr(path)
    elif ext == ".exr":
        try:
            import imageio
            imageio.formats["EXR"]  # raises when no EXR plugin is available
            img = np.asarray(imageio.imread(path))
        except Exception as e:
            raise _lib.IronError("%s: imageio has no EXR plugin here (%s); convert the map to .hdr or .npy" % (path, e))
    else:
        raise _lib.IronError("%s: an environment map is .npy, .hdr or .exr" % path)
    img = np.asarray(img, dtype=np.float32)
    if img.ndim != 3 or img.shape[2] < 3:
        raise _lib.IronError("%s: expected [He, We, 3], got %s" % (path, img.shape))
    return np.ascontiguousarray(img[:, :, :3])
