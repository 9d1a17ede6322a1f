"""The RoI case tables shared by tests/test_roi_bound_host.py (which checks the conditions on them, on the reference alone) and
tests/test_gpu_roi_exact.py (which runs the kernels on them).  Boxes are in input pixels at spatial_scale 1/16; a table is a list of
(name, image, x0, y0, x1, y1), sorted by image.  Not a conftest."""
import torch

SCALE = 1.0 / 16
PH = PW = 14
MAPS = ((13, 21), (40, 67))             # feature maps H x W of table F
SEED = {(13, 21): 11, (40, 67): 12}     # seeds of the random boxes for which the table conditions hold (test_roi_bound_host.py)
E = 2.0 ** -6                           # 2^-10 feature pixels

# Dyadic edge boxes on the 13 x 21 map: every f32 operation of the geometry is exact, so the window tests are decided exactly.
# (name, box, aligned, sampling_ratio, ph = pw).  With bins of one pixel and one sample per bin, bin (i, j) samples the point
# (y0 + i + 0.5, x0 + j + 0.5); x0 = 2 puts the x samples half way between columns 2 + j and 3 + j.
# The "_a" twins give the same geometry under aligned = True (corners 8 pixels further: y0 = corner / 16 - 0.5).
EDGE = [
    ("at_minus1", (32.0, -24.0, 256.0, 200.0), False, 0, 14),            # y samples -1, 0, .., 12: the first is counted (row 0)
    ("outside_minus1", (32.0, -24.0 - E, 256.0, 200.0 - E), False, 0, 14),  # -1 - 2^-10: dropped; then -2^-10 (clamped), 1 - 2^-10, ..
    ("at_L", (32.0, 8.0, 256.0, 232.0), False, 0, 14),                    # y samples 1 .. 14: 13 = L counted (row 12), 14 dropped
    ("top_pixel", (32.0, 0.0, 256.0, 224.0), False, 0, 14),               # y samples 0.5 .. 13.5: 12.5 snaps to row 12, 13.5 dropped
    ("at_minus1_a", (40.0, -16.0, 264.0, 208.0), True, 0, 14),
    ("outside_minus1_a", (40.0, -16.0 - E, 264.0, 208.0 - E), True, 0, 14),
    ("at_L_a", (40.0, 16.0, 264.0, 240.0), True, 0, 14),
    ("top_pixel_a", (40.0, 8.0, 264.0, 232.0), True, 0, 14),
    ("empty_adaptive", (48.0, 48.0, 48.0, 48.0), True, 0, 14),            # a 0 x 0 grid: zeros
    ("empty_sr2", (48.0, 48.0, 48.0, 48.0), True, 2, 14),                 # every sample at (2.5, 2.5)
    ("outside_image", (400.0, 300.0, 624.0, 524.0), False, 0, 14),        # x0 = 25 > W: every sample dropped
    ("subpixel_floored", (40.0, 40.0, 44.0, 44.0), False, 0, 4),          # 0.25 x 0.25 pixels floored to 1 x 1: bins of 1/4
    ("inverted", (504.0, 40.0, 56.0, 264.0), True, 0, 14),                # x1 < x0 by 28 feature pixels: gw = ceil(-2) = -2: zeros
]


def _grid_box(H, W, gh, gw):
    """a box (aligned = True) whose adaptive grid is gh x gw: rh = 14 gh - 7 feature pixels, anchored so that it overlaps the map"""
    rh, rw = 14.0 * gh - 7.0, 14.0 * gw - 7.0
    y0 = 1.25 if rh <= H - 2 else (H - rh) / 2          # (a grid larger than the map is centred on it)
    x0 = 2.75 if rw <= W - 3 else (W - rw) / 2
    return ((x0 + 0.5) * 16, (y0 + 0.5) * 16, (x0 + rw + 0.5) * 16, (y0 + rh + 0.5) * 16)


def threshold_boxes(H, W):
    """one box per dispatch threshold of k_roi_align_fwd_rows (and of the tap kernel's LDS tables), named after what it reaches:
      gh 1..5     merged feature rows per bin row on both sides of the prefetch form's PF = 4 (nrow <= 4 / rload)
      gh 8 | 9    2 ny > ROW_MAXY = 32 for the pooled-only output (ny = 2 gh)
      gh 16 | 17  the same for the crops (ny = gh)
      gw 18 | 19  nx = 14 gw > ROI_MAXS = 256
      whole, wide_sr2   bins wider than 2 (4) pixels: under sampling_ratio = 2 the slide moves more than one column per sample"""
    out = [(f"gh{g}", _grid_box(H, W, g, 2)) for g in (1, 2, 3, 4, 5, 8, 9, 16, 17)]
    out += [(f"gw{g}", _grid_box(H, W, 2, g)) for g in (1, 2, 18, 19)]
    out.append(("whole", (0.0, 0.0, W * 16.0, H * 16.0)))
    out.append(("wide_sr2", (8.0, 24.0, 8.0 + 63 * 16.0, 24.0 + 35 * 16.0)))
    return out


def random_boxes(H, W, n, seed):
    g = torch.Generator().manual_seed(seed)
    r = torch.rand(n, 6, generator=g)
    x0 = r[:, 0] * (W * 16 + 120) - 60
    y0 = r[:, 1] * (H * 16 + 120) - 60
    w = 6 + r[:, 2] ** 2 * 600
    h = 6 + r[:, 3] ** 2 * 500
    return [(f"rand{i}", (float(x0[i]), float(y0[i]), float(x0[i] + w[i]), float(y0[i] + h[i]))) for i in range(n)]


def _assemble(named, N, extra=()):
    """spread the boxes over N images (round robin), sort by image, append ``extra`` (name, image, box) rows"""
    rows = [(name, i % N, *box) for i, (name, box) in enumerate(named)]
    rows.sort(key=lambda r: r[1])
    return rows + list(extra)


def table_F(H, W, N=2, n_random=30, seed=None):
    """table F of one map: random boxes, the dyadic edge boxes, one box per threshold, and one RoI naming image N (last)"""
    named = random_boxes(H, W, n_random, SEED[(H, W)] if seed is None else seed)
    named += [(n, b) for n, b, *_ in EDGE] + threshold_boxes(H, W)
    return _assemble(named, N, [("batch_index_N", N, 64.0, 48.0, 200.0, 160.0)])


def table_bench(H=50, W=84, counts=(96, 70), seed=5):
    """boxes with the training workload's statistics: clipped to the image, sides 2 .. 16 feature pixels (mean 9)"""
    g = torch.Generator().manual_seed(seed)
    rows = []
    for n, cnt in enumerate(counts):
        r = torch.rand(cnt, 4, generator=g)
        w, h = 16 * (2 + 14 * r[:, 2]), 16 * (2 + 14 * r[:, 3])
        x0, y0 = r[:, 0] * (W * 16 - w), r[:, 1] * (H * 16 - h)
        rows += [(f"bench{n}_{i}", n, float(x0[i]), float(y0[i]), float(x0[i] + w[i]), float(y0[i] + h[i])) for i in range(cnt)]
    return rows


def table_counts(H, W, counts, seed):
    """random boxes, counts[n] of them in image n (the ballot loop of the gather backward takes 64 RoIs at a time)"""
    rows = []
    for n, cnt in enumerate(counts):
        rows += [(f"img{n}_{name}", n, *box) for name, box in random_boxes(H, W, cnt, seed + n)]
    return rows


def rois_tensor(rows, device="cpu"):
    return torch.tensor([[float(r[1]), *r[2:]] for r in rows], dtype=torch.float32, device=device).reshape(-1, 5)


def names(rows):
    return [r[0] for r in rows]


def roi_start(rows, N, device="cpu"):
    b = torch.tensor([r[1] for r in rows], dtype=torch.int64)
    return torch.searchsorted(b, torch.arange(N + 1)).to(torch.int32).to(device)
