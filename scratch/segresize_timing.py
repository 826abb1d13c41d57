"""Timing of the two resizes of `segmentor_width_size` on the GPU: sam6d_hip.amg.resize_masks against the
parent's route, masks.float() followed by F.interpolate, and amg.resize_image against resize_image_eager on the device and on the
host (the parent's own route is cv2.resize on the host, which does not run where cv2 is missing).  Paths alternated in one process,
device events (wall clock for host work), median of repeated runs after two warm-ups.  Then generate_masks end to end with the stub
network (tests/sam_amg_stub.py), 1024 points on a 1080 x 1920 image at segmentor_width_size 640, hip_resize on and off; the off leg
needs a host resize, for which resize_image_eager on the CPU stands in for cv2.resize.

    python scratch/segresize_timing.py [--reps 9]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "openvino-sam-6d_amd"), os.path.join(ROOT, "openvino-sam-6d_amd", "ism")]
from sam6d_hip import amg  # noqa: E402
from tests.sam_amg_stub import StubSam, encode_image  # noqa: E402

DEV = "cuda:0"
THREADS = torch.get_num_threads()
HBM_WRITE = 6.1e12  # bytes / s: plain streaming stores on MI355X (6.0 - 6.2 TB/s measured)


def device_ms(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    res = fn()
    b.record()
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    del res
    return a.elapsed_time(b), peak


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    del res
    return (time.perf_counter() - t0) * 1e3, 0.0


def tick():
    torch.cuda.synchronize()
    return time.perf_counter()


def alternate(paths, reps, timer=device_ms):
    for _ in range(2):
        for fn in paths.values():
            timer(fn)
    t = {k: [] for k in paths}
    for _ in range(reps):  # alternated: every path sees the same clocks
        for k, fn in paths.items():
            t[k].append(timer(fn))
    return {k: (statistics.median(x[0] for x in v), min(x[0] for x in v), max(x[0] for x in v), max(x[1] for x in v)) for k, v in t.items()}


def report(name, res, extra=""):
    for k, (med, lo, hi, peak) in res.items():
        print("%-44s %-14s median %9.3f ms  (min %9.3f, max %9.3f)  peak %8.1f MiB%s" % (name, k, med, lo, hi, peak, extra))


def blobs(K, h, w):
    g = torch.Generator().manual_seed(K + h)
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    cy, cx, r = torch.rand(K, generator=g) * h, torch.rand(K, generator=g) * w, 20 + torch.rand(K, generator=g) * h / 3
    return ((yy[None] - cy[:, None, None]) ** 2 + (xx[None] - cx[:, None, None]) ** 2 <= r[:, None, None] ** 2).to(DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()

    for (h, w), (H, W) in (((360, 640), (1080, 1920)), ((480, 640), (960, 1280))):
        for K in (50, 200):
            m = blobs(K, h, w)
            paths = {"float+interp": lambda: F.interpolate(m.float().unsqueeze(1), size=(H, W), mode="bilinear", align_corners=False)[:, 0],
                     "resize_masks": lambda: amg.resize_masks(m, (H, W)),
                     "resize_masks (2)": lambda: amg.resize_masks(m, (H, W))}  # the second of two in a row: not behind F.interpolate's writes
            floor = K * H * W * 4 / HBM_WRITE * 1e3
            res = alternate(paths, args.reps)
            report("masks %3d x %d x %d -> %d x %d" % (K, h, w, H, W), res, "  write floor %.3f ms" % floor)
            print("%-44s ratio float+interp / resize_masks: %.2f" % ("", res["float+interp"][0] / res["resize_masks"][0]))
            del m
            torch.cuda.empty_cache()

    for (H, W) in ((1080, 1920), (960, 1280)):
        img = np.random.default_rng(H).integers(0, 256, (H, W, 3), dtype=np.uint8)
        size = amg.resized_shape((H, W), 640)
        host, d = torch.from_numpy(img), torch.from_numpy(img).to(DEV)
        report("image %d x %d -> %d x %d" % (H, W, size[0], size[1]),
               alternate({"resize_image": lambda: amg.resize_image(d, size), "eager (device)": lambda: amg.resize_image_eager(d, size)}, args.reps))
        report("image %d x %d -> %d x %d" % (H, W, size[0], size[1]),
               alternate({"upload+resize": lambda: amg.resize_image(host.to(DEV), size), "eager (host)": lambda: amg.resize_image_eager(host, size)},
                         args.reps, wall_ms))

    import importlib
    mod = importlib.import_module("model.sam")

    class HostEagerResize(mod.CustomSamAutomaticMaskGenerator):
        """hip_resize off, with resize_image_eager on the CPU standing in for cv2.resize."""

        def preprocess_resize(self, image):
            torch.set_num_threads(1)  # (with more, the pool's threads spin into the next call and slow whichever route follows)
            try:
                return amg.resize_image_eager(torch.from_numpy(image), self._resized_shape(image.shape[:2])).numpy()
            finally:
                torch.set_num_threads(THREADS)

    image = np.random.default_rng(1).integers(0, 256, (1080, 1920, 3), dtype=np.uint8)
    sam = StubSam(DEV)
    for min_area in (0, 50):
        kw = dict(encode_image=encode_image, segmentor_width_size=640, min_mask_region_area=min_area)
        on = mod.CustomSamAutomaticMaskGenerator(sam, hip_resize=True, **kw)
        off = HostEagerResize(sam, hip_resize=False, **kw)
        n = on.generate_masks(image)["masks"].shape[0], off.generate_masks(image)["masks"].shape[0]
        res = alternate({"hip_resize on": lambda: on.generate_masks(image), "off (host eager)": lambda: off.generate_masks(image)}, args.reps, wall_ms)
        report("generate_masks 1080 x 1920, min_area %d" % min_area, res, "  survivors %d / %d" % n)
        # the same call leg by leg (a synchronisation between the legs): whole-call wall times depend on which route runs behind the
        # host resize, whose CPU threads keep spinning into the next call
        legs = {k: [] for k in ("hip_resize on", "off (host eager)")}
        for _ in range(args.reps + 2):
            for k, g in (("hip_resize on", on), ("off (host eager)", off)):
                t = [tick()]
                small = g.preprocess_resize(image)
                t.append(tick())
                data = g._generate_masks(small, torch.bool if g.hip_resize or min_area > 0 else torch.float32)
                if min_area > 0:
                    data = g.postprocess_small_regions(data, min_area, 0.7)
                t.append(tick())
                data = g.postprocess_resize(data, image.shape[:2])
                t.append(tick())
                del data
                legs[k].append([(b - a) * 1e3 for a, b in zip(t, t[1:])])
        for k, v in legs.items():
            print("%-44s %-16s legs, medians: resize in %8.3f ms, generate %8.3f ms, resize out %8.3f ms" % (
                "", k, *(statistics.median(x[i] for x in v[2:]) for i in range(3))))


if __name__ == "__main__":
    main()
