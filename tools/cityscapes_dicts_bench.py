#!/usr/bin/env python
"""Start-up cost of the Cityscapes dataset dicts: N synthetic 2048x1024 instanceIds PNGs (generated from a seed), then wall time of
  * decode    -- the 8-thread PNG decode of cityscapes.files_to_dicts,
  * extract   -- the kernel on the decoded maps (upload, cddmsl_instance_boxes, readback; batches of 8),
  * dicts     -- cityscapes.files_to_dicts end to end (decode + extract + annotation rules),
  * numpy     -- the reference's per-id compare + np.nonzero (cityscapes.py:501-540) on the host, one thread, same maps,
and checks that kernel and host records agree.  Prints one JSON line.

    python tools/cityscapes_dicts_bench.py --n 32 --dir /tmp/city_maps
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_map(rng, h=1024, w=2048, n=40):
    """stuff ids in 32-pixel blocks, then n ragged rectangles of thing ids (k * 1000 + j) and a few crowd ids"""
    m = rng.randint(0, 24, (h // 32 + 1, w // 32 + 1)).repeat(32, 0).repeat(32, 1)[:h, :w].astype(np.uint16)
    for j in range(n):
        iid = int(rng.choice([24, 26, 33])) if j % 10 == 9 else int(rng.randint(24, 34)) * 1000 + j
        y0, x0 = rng.randint(0, h), rng.randint(0, w)
        y1, x1 = min(h, y0 + rng.randint(8, 300)), min(w, x0 + rng.randint(8, 400))
        m[y0:y1, x0:x1][rng.rand(y1 - y0, x1 - x0) < 0.9] = iid
    return m


def numpy_records(inst_image):
    out = []
    for iid in np.unique(inst_image[inst_image >= 24]):
        ys, xs = np.nonzero(np.asarray(inst_image == iid, dtype=np.uint8, order="F"))
        out.append((int(iid), int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()), int(len(ys))))
    return np.array(out, dtype=np.int32).reshape(-1, 6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--dir", required=True)
    a = ap.parse_args()
    import torch
    from PIL import Image
    from cddmsl_amd import cityscapes as cs, hip
    os.makedirs(a.dir, exist_ok=True)
    rng = np.random.RandomState(0)
    paths = []
    for i in range(a.n):
        p = os.path.join(a.dir, f"frame{i:04d}_gtFine_instanceIds.png")
        Image.fromarray(synthetic_map(rng)).save(p)
        paths.append(p)
    files = [(p, None, p) for p in paths]
    cs.files_to_dicts(files[:2])                       # warm-up: library load, first launches
    torch.cuda.synchronize()

    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=8) as pool:
        maps = list(pool.map(cs.read_instance_map, paths))
    t1 = time.perf_counter()
    recs = []
    for s in range(0, a.n, 8):
        recs += hip.instance_boxes_host(torch.from_numpy(np.stack(maps[s:s + 8])).cuda())
    t2 = time.perf_counter()
    cs.files_to_dicts(files)
    t3 = time.perf_counter()
    ref = [numpy_records(m) for m in maps]
    t4 = time.perf_counter()
    assert all(np.array_equal(x, y) for x, y in zip(recs, ref)), "kernel and numpy records differ"
    print(json.dumps({"n_maps": a.n, "map": "2048x1024 uint16", "decode_s": round(t1 - t0, 4), "extract_s": round(t2 - t1, 4),
                      "dicts_s": round(t3 - t2, 4), "numpy_s": round(t4 - t3, 4),
                      "instances_per_map": round(float(np.mean([len(r) for r in ref])), 1)}))


if __name__ == "__main__":
    main()
