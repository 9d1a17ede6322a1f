"""Paired (labeled image + domain-translated twin) VOC data pipeline -> device batches.

Follows the reference's input side:
  * dataset dicts: ``load_voc_DG_instances`` data/datasets/pascal_voc.py:98-171 (boxes XYXY with xmin/ymin - 1, "difficult"
    objects kept, twin at ``<dirname>/../<dt_data>/<VOC2007|VOC2012>/JPEGImages/<id>.jpg`` for the training splits);
  * mapper: ``DatasetMapper.__call__`` data/dataset_mapper.py:126-217 -- read both images (RGB/BGR, EXIF orientation), ONE
    sampled transform list (``ResizeShortestEdge`` + ``RandomFlip``, detection_utils.py:590-614, augmentation_impl.py:149-199)
    applied to both images and to the boxes, boxes clipped to the image, empty boxes dropped (detection_utils.py:257-317,393-430);
  * sampler / batching: ``TrainingSampler`` samplers/distributed_sampler.py:12-58 (one seeded infinite permutation stream, rank r
    takes every world-th index), ``AspectRatioGroupedDataset`` data/common.py:152-186 (a batch holds only landscape or only
    portrait images), per-rank batch = IMS_PER_BATCH / world (data/build.py:280-287);
  * batch item: ``{"image": u8 [3,H,W], "image_trgt": u8 [3,H,W], "instances": Instances(gt_boxes, gt_classes), "height",
    "width", "file_name", "image_id"}`` -- the contract ``GeneralizedRCNN.forward`` reads.

Host -> device: images leave the loader as pinned uint8 tensors and are copied with ``non_blocking=True``; normalisation and
padding happen on the GPU (``cddmsl_preprocess``).  Resizing is PIL bilinear on uint8, exactly the call the reference makes
(``Image.resize((w, h), BILINEAR)``, transforms/transform.py ResizeTransform); the reference's transform classes derive from
fvcore, which is not installed here, so their numerics are pinned by that shared PIL call, not by a fixture (parity unpinned).

``DATALOADER.DEVICE_RESIZE`` (default off) moves resize, flip, HWC -> CHW and RGB -> BGR into ONE HIP launch per batch on the staging
stream (``cddmsl_resize_batch_u8``, Pillow's resample bit for bit): the mapper then only decodes and records what is left to do, and
``DeviceBatches`` hands out the same bytes as the host path.

``INPUT.COLOR_JITTER`` (default off; augment.py) varies the photometry of the training images after crop, resize and flip: in the mapper
(numpy) on the host path, in one more HIP launch per batch (``cddmsl_color_jitter_batch_u8``) behind the resize on the device path --
the same bytes either way.
"""
import os
import xml.etree.ElementTree as ET
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .augment import ColorJitter, color_jitter_u8
from .config import check_color_jitter
from .evaluation import VOC_CLASS_NAMES
from .structures import Boxes, Instances


# ------------------------------------------------------------------------------------------------ dataset dicts
def load_voc_instances(dirname: str, split: str, class_names: Sequence[str] = VOC_CLASS_NAMES, dt_data: Optional[str] = None) -> List[Dict]:
    with open(os.path.join(dirname, "ImageSets", "Main", split + ".txt")) as f:
        fileids = [l.strip() for l in f if l.strip()]
    paired = split in ("train", "trainval") and dt_data is not None
    voc_dir = "VOC2007" if "VOC2007" in os.path.join(dirname, "JPEGImages") else "VOC2012"
    dicts = []
    for fid in fileids:
        root = ET.parse(os.path.join(dirname, "Annotations", fid + ".xml")).getroot()
        r = {"file_name": os.path.join(dirname, "JPEGImages", fid + ".jpg"), "image_id": fid,
             "height": int(root.findall("./size/height")[0].text), "width": int(root.findall("./size/width")[0].text)}
        if paired:
            r["data_dt_file_name"] = os.path.join(dirname, "..", dt_data, voc_dir, "JPEGImages", fid + ".jpg")
        anns = []
        for obj in root.findall("object"):
            bb = obj.find("bndbox")
            box = [float(bb.find(k).text) for k in ("xmin", "ymin", "xmax", "ymax")]
            box[0] -= 1.0                       # 1-based inclusive pixel indices -> continuous coordinates
            box[1] -= 1.0
            anns.append({"category_id": list(class_names).index(obj.find("name").text), "bbox": box})
        r["annotations"] = anns
        dicts.append(r)
    return dicts


# ------------------------------------------------------------------------------------------------ image I/O + transforms
def read_image(path, fmt="RGB"):
    """detection_utils.py:171-190: PIL decode, EXIF orientation, RGB or BGR uint8 HWC"""
    from PIL import Image, ImageOps
    with open(path, "rb") as f:
        img = Image.open(f)
        img = ImageOps.exif_transpose(img)
        arr = np.asarray(img.convert("RGB"))
    return arr[:, :, ::-1] if fmt == "BGR" else arr


def shortest_edge_size(h, w, size, max_size):
    """augmentation_impl.py:188-198 -> (new_h, new_w)"""
    scale = size * 1.0 / min(h, w)
    newh, neww = (size, scale * w) if h < w else (scale * h, size)
    if max(newh, neww) > max_size:
        scale = max_size * 1.0 / max(newh, neww)
        newh, neww = newh * scale, neww * scale
    return int(newh + 0.5), int(neww + 0.5)


def resize_image(img, newh, neww):
    """ResizeTransform.apply_image for uint8: PIL bilinear"""
    from PIL import Image
    if img.shape[:2] == (newh, neww):
        return img
    return np.asarray(Image.fromarray(img).resize((neww, newh), Image.BILINEAR))


DEVICE_RESIZE_KEY = "device_resize"      # a sample's record of the resize / mirror / channel reversal still to be done on the device


class DatasetMapper:
    """Dataset dict -> model input dict; the random draws come from ``rng`` in the reference's order: the crop window (INPUT.CROP,
    ``RandomCrop`` augmentation_impl.py:367-399), the short edge (``choice`` or, with MIN_SIZE_TRAIN_SAMPLING "range", ``randint``),
    then the flip, then INPUT.COLOR_JITTER's (``augment.ColorJitter.draw_pair``; none when the block is off or no operation is active)
    -- a ``RandomState(s)`` reproduces ``np.random.seed(s)`` on the reference.  With the shipped defaults that is one ``rng.choice`` and
    one ``rng.uniform`` per sample.  The test mapper resizes only (``build_augmentation(cfg, False)``)."""

    CROP_TYPES = ("relative_range", "relative", "absolute", "absolute_range")

    def __init__(self, cfg, is_train=True, rng: Optional[np.random.RandomState] = None):
        i = cfg.INPUT
        self.is_train, self.fmt = is_train, i.FORMAT
        self.min_sizes = list(i.MIN_SIZE_TRAIN) if is_train else [i.MIN_SIZE_TEST]
        self.max_size = i.MAX_SIZE_TRAIN if is_train else i.MAX_SIZE_TEST
        self.size_range, self.flip, self.crop_type, self.crop_size, self.jitter = False, 0, None, None, None
        if is_train:
            block = check_color_jitter(cfg)
            jitter = ColorJitter(block) if block is not None else None
            self.jitter = jitter if jitter is not None and jitter.active else None      # (no active operation: no draws at all)
            style, flip, crop = i.get("MIN_SIZE_TRAIN_SAMPLING", "choice"), i.get("RANDOM_FLIP", "horizontal"), i.get("CROP") or {}
            if style not in ("choice", "range"):
                raise ValueError(f"INPUT.MIN_SIZE_TRAIN_SAMPLING must be 'choice' or 'range', not {style!r}")
            if style == "range" and len(self.min_sizes) != 2:
                raise ValueError(f"INPUT.MIN_SIZE_TRAIN must hold two values (min, max) with INPUT.MIN_SIZE_TRAIN_SAMPLING 'range', not {tuple(self.min_sizes)}")
            if flip not in ("horizontal", "vertical", "none"):
                raise ValueError(f"INPUT.RANDOM_FLIP must be 'horizontal', 'vertical' or 'none', not {flip!r}")
            self.size_range = style == "range"
            self.flip = {"none": 0, "horizontal": 1, "vertical": 2}[flip]         # the device record's (and the kernel's) flip code
            if crop.get("ENABLED", False):
                self.crop_type, self.crop_size = crop.get("TYPE", "relative_range"), tuple(crop.get("SIZE", (0.9, 0.9)))
                if self.crop_type not in self.CROP_TYPES:
                    raise ValueError(f"INPUT.CROP.TYPE must be one of {self.CROP_TYPES}, not {self.crop_type!r}")
                if len(self.crop_size) != 2:
                    raise ValueError(f"INPUT.CROP.SIZE must hold two values, not {self.crop_size}")
        self.device_resize = bool(cfg.DATALOADER.get("DEVICE_RESIZE", False))
        self.rng = rng or np.random.RandomState()

    def _crop_window(self, h, w):
        """``RandomCrop.get_crop_size`` + ``get_transform`` -> (y0, x0, ch, cw)"""
        t, s = self.crop_type, self.crop_size
        if t == "relative":
            ch, cw = int(h * s[0] + 0.5), int(w * s[1] + 0.5)
        elif t == "relative_range":
            s32 = np.asarray(s, dtype=np.float32)                   # (the reference rounds SIZE to float32, then mixes in float64)
            fh, fw = s32 + self.rng.rand(2) * (1 - s32)
            ch, cw = int(h * fh + 0.5), int(w * fw + 0.5)
        elif t == "absolute":
            ch, cw = min(int(s[0]), h), min(int(s[1]), w)
        else:                                                       # "absolute_range": SIZE is (min, max) for both axes
            assert s[0] <= s[1], "INPUT.CROP.SIZE of 'absolute_range' is (min, max)"
            ch = int(self.rng.randint(min(h, s[0]), min(h, s[1]) + 1))
            cw = int(self.rng.randint(min(w, s[0]), min(w, s[1]) + 1))
        assert 0 < ch <= h and 0 < cw <= w, f"INPUT.CROP.SIZE {s} ({t}) gives a {ch} x {cw} crop of a {h} x {w} image"
        y0 = int(self.rng.randint(h - ch + 1))
        x0 = int(self.rng.randint(w - cw + 1))
        return y0, x0, ch, cw

    def __call__(self, d: Dict) -> Dict:
        d = dict(d)
        fmt = "RGB" if self.device_resize else self.fmt            # (the device reverses the channels while it resizes)
        img = read_image(d["file_name"], fmt)
        assert img.shape[:2] == (d["height"], d["width"]), f"{d['file_name']}: image size differs from its annotation"
        twin = read_image(d["data_dt_file_name"], fmt) if "data_dt_file_name" in d else None
        if twin is not None:
            assert twin.shape[:2] == img.shape[:2], f"{d['data_dt_file_name']}: twin size differs"
        y0 = x0 = 0
        if self.crop_type is not None:                             # one window for the image and its twin, in front of the resize
            y0, x0, ch, cw = self._crop_window(*img.shape[:2])
            img = img[y0:y0 + ch, x0:x0 + cw]
            if twin is not None:
                twin = twin[y0:y0 + ch, x0:x0 + cw]
        h, w = img.shape[:2]                                       # (the cropped size; d["height"] / d["width"] stay the original's)
        size = int(self.rng.randint(self.min_sizes[0], self.min_sizes[1] + 1) if self.size_range else self.rng.choice(self.min_sizes))
        newh, neww = shortest_edge_size(h, w, size, self.max_size) if size else (h, w)
        flip = bool(self.flip and self.rng.uniform() < 0.5) and self.flip      # False, or the code of the configured mirror

        jit, jit_twin = self.jitter.draw_pair(self.rng, twin is not None) if self.jitter is not None else (None, None)

        def tf(a, jitter=None):
            a = resize_image(a, newh, neww)
            a = a[:, ::-1] if flip == 1 else (a[::-1] if flip == 2 else a)
            if jitter:
                a = color_jitter_u8(a, jitter, self.fmt == "BGR")
            return a

        if self.device_resize:
            # DATALOADER.DEVICE_RESIZE: the decoded (and cropped) [h, w, 3] RGB arrays go on as they are, with a record of what is still
            # to do; DeviceBatches resizes, mirrors, reverses and transposes the whole batch in one kernel launch.  Only the coefficient
            # tables of the changed axes are built here -- in the worker, where the PIL resize used to run.  "flip" is the kernel's
            # code: False (0) none, 1 left-right, 2 top-bottom
            from .resample import packed_table
            d[DEVICE_RESIZE_KEY] = {"size": (newh, neww), "flip": flip, "reverse_channels": self.fmt == "BGR",
                                    "xtab": packed_table(w, neww) if neww != w else None,
                                    "ytab": packed_table(h, newh) if newh != h else None}
            if jit or jit_twin:                                      # INPUT.COLOR_JITTER's draws: applied behind the resize, one launch per batch
                d[DEVICE_RESIZE_KEY]["jitter"] = {"image": jit, "image_trgt": jit_twin}
            d["image"] = torch.from_numpy(np.array(img, order="C"))     # (a copy: PIL hands out a read-only buffer; of the window only)
            if twin is not None:
                d["image_trgt"] = torch.from_numpy(np.array(twin, order="C"))
        else:
            d["image"] = torch.from_numpy(np.ascontiguousarray(tf(img, jit).transpose(2, 0, 1)))
            if twin is not None:
                d["image_trgt"] = torch.from_numpy(np.ascontiguousarray(tf(twin, jit_twin).transpose(2, 0, 1)))
        anns = d.pop("annotations", None)
        if not self.is_train or anns is None:
            return d
        anns = [a for a in anns if not a.get("iscrowd", 0)]                                        # dataset_mapper.py:203
        boxes = np.asarray([a["bbox"] for a in anns], dtype=np.float64).reshape(-1, 4)
        if x0 or y0:
            boxes = boxes - np.array([x0, y0, x0, y0], dtype=np.float64)               # CropTransform.apply_coords
        boxes = boxes * np.array([neww / w, newh / h, neww / w, newh / h])            # ResizeTransform.apply_coords
        if flip == 1:
            boxes = np.stack([neww - boxes[:, 2], boxes[:, 1], neww - boxes[:, 0], boxes[:, 3]], axis=1)   # HFlip + re-sort corners
        elif flip == 2:
            boxes = np.stack([boxes[:, 0], newh - boxes[:, 3], boxes[:, 2], newh - boxes[:, 1]], axis=1)   # VFlip + re-sort corners
        boxes = np.minimum(boxes, np.array([neww, newh, neww, newh], dtype=np.float64)).clip(min=0)       # transform_instance_annotations
        gt = Boxes(torch.from_numpy(boxes.astype(np.float32)))
        cls = torch.tensor([a["category_id"] for a in anns], dtype=torch.int64)
        keep = gt.nonempty(threshold=1e-5)                                                                  # filter_empty_instances
        d["instances"] = Instances((newh, neww), gt_boxes=gt[keep], gt_classes=cls[keep])
        return d


# ------------------------------------------------------------------------------------------------ sampling, batching, device
class TrainingSampler:
    """Infinite stream of indices: permutations drawn from one seeded generator shared by all ranks, sharded rank::world."""

    def __init__(self, size, shuffle=True, seed=0, rank=0, world=1):
        self.size, self.shuffle, self.seed, self.rank, self.world = size, shuffle, int(seed), rank, world

    def __iter__(self):
        g = torch.Generator().manual_seed(self.seed)
        pos = 0
        while True:
            order = torch.randperm(self.size, generator=g).tolist() if self.shuffle else list(range(self.size))
            for i in order:
                if pos % self.world == self.rank:
                    yield i
                pos += 1


class _Mapped(torch.utils.data.IterableDataset):
    def __init__(self, dicts, mapper, sampler):
        self.dicts, self.mapper, self.sampler = dicts, mapper, sampler

    def __iter__(self):
        info = torch.utils.data.get_worker_info()
        wid, nw = (info.id, info.num_workers) if info is not None else (0, 1)
        if info is not None:                                      # decorrelate the augmentation streams of the workers
            self.mapper.rng = np.random.RandomState((self.sampler.seed * 1009 + self.sampler.rank * 101 + wid) % (2 ** 31))
        for n, idx in enumerate(self.sampler):
            if n % nw == wid:
                yield self.mapper(self.dicts[idx])


def _worker_init(_):
    torch.set_num_threads(1)          # a worker decodes / resizes with PIL: no intra-op pool per worker process


def aspect_ratio_batches(stream, batch_size):
    """data/common.py:152-186: two buckets (w > h, w <= h); a bucket is emitted when it holds batch_size samples"""
    buckets = ([], [])
    for d in stream:
        # (a sample still to be resized on the device is bucketed by its target size: what this sees after a host resize)
        h, w = d[DEVICE_RESIZE_KEY]["size"] if DEVICE_RESIZE_KEY in d else d["image"].shape[1:]
        b = buckets[0 if w > h else 1]
        b.append(d)
        if len(b) == batch_size:
            yield b[:]
            del b[:]


class DeviceBatches:
    """Iterator of per-rank batches resident on ``device``.

    CUDA: a background thread takes the host batches as they come, packs every image of a batch (and its twin) into ONE pinned
    staging buffer from a small pool, sends it with one non-blocking copy on a side stream (boxes and classes likewise, one copy
    each) and hands the device views over together with an event; ``__next__`` makes the caller's stream wait for that event --
    the host never blocks on a copy, and batch i+1 is staged while the GPU runs step i.  (Round 3 measurement,
    tools/loader_bench.py: ``tensor.pin_memory()`` per image -- a pinned allocation each -- capped the loader at ~139 samples/s
    whatever the worker count, below the 152 samples/s the step consumes.)"""

    def __init__(self, batches, device, prefetch=2, max_batch_bytes=0):
        self.batches, self.device = iter(batches), torch.device(device)
        self._thread = None
        if self.device.type == "cuda":
            import atexit
            import queue
            import threading
            import weakref
            self._q = queue.Queue(maxsize=prefetch)
            self._stop = False
            self._stream = torch.cuda.Stream(self.device)
            self._free, self._busy = [], []                # pinned staging buffers: reusable / (event, buffer) still being read
            self._cap = int(max_batch_bytes)               # a pinned allocation costs tens of ms: buffers are sized for the largest batch
            self._thread = threading.Thread(target=self._run, daemon=True)
            self._thread.start()
            ref = weakref.ref(self)
            atexit.register(lambda: ref() is not None and ref().close())   # the thread must be gone before the runtime is torn down

    def __iter__(self):
        return self

    def close(self):
        """drop the batch stream (shuts the DataLoader's worker processes down with it)"""
        if self._thread is not None:
            self._stop = True
            try:
                while True:
                    self._q.get_nowait()
            except Exception:
                pass
            self._thread.join(timeout=5.0)
            self._thread = None
        self.batches = iter(())
        import gc
        gc.collect()

    # ---------------------------------------------------------------- staging thread
    def _pinned(self, nbytes):
        still = []
        for ev, b in self._busy:                           # buffers whose copy has completed go back to the pool
            if ev.query():
                self._free.append(b)
            else:
                still.append((ev, b))
        self._busy = still
        for i, b in enumerate(self._free):
            if b.numel() >= nbytes:
                return self._free.pop(i)
        self._cap = max(self._cap, int(nbytes * 1.25) + 4096)
        self._free = []                                    # (smaller ones would never be picked again)
        return torch.empty(self._cap, dtype=torch.uint8, pin_memory=True)

    def _stage(self, batch):
        """host batch -> (device batch, event, device buffers): every image, twin, box and class tensor of the batch packed into one
        pinned buffer (256-byte slots) and sent with ONE copy.  Samples that carry a DATALOADER.DEVICE_RESIZE record arrive as decoded
        [h, w, 3] images: those and their coefficient tables (one per distinct (in, out) axis pair of the batch) ride in the same
        copy, and ONE kernel launch on the staging stream resizes / mirrors / transposes them into a second device buffer whose
        [3, newh, neww] views are handed out; the event is recorded behind the kernel."""
        items = []                                         # (sample index, field, tensor)
        recs, tabs = {}, {}                                # sample index -> record; (insize, outsize) -> index of that table in items
        for i, d in enumerate(batch):
            if DEVICE_RESIZE_KEY in d:
                recs[i] = d[DEVICE_RESIZE_KEY]
            for k in ("image", "image_trgt"):
                if k in d:
                    items.append((i, k, d[k]))
            if "instances" in d:
                items.append((i, "gt_boxes", d["instances"].gt_boxes.tensor.contiguous()))
                items.append((i, "gt_classes", d["instances"].gt_classes.contiguous()))
        for i, rec in recs.items():
            h, w = batch[i]["image"].shape[:2]
            for ax, insize, outsize in (("xtab", w, rec["size"][1]), ("ytab", h, rec["size"][0])):
                if rec[ax] is not None and (insize, outsize) not in tabs:
                    tabs[(insize, outsize)] = len(items)
                    items.append((i, ax, torch.as_tensor(rec[ax][0])))      # (numpy from the mapper, a tensor through DataLoader workers)
        sizes = [(t.numel() * t.element_size() + 255) // 256 * 256 for _, _, t in items]
        buf = self._pinned(sum(sizes))
        off, slots = 0, []
        for (i, k, t), n in zip(items, sizes):
            nb = t.numel() * t.element_size()
            if nb:
                buf[off:off + nb].view(t.dtype).view(t.shape).copy_(t)
            slots.append((i, k, off, nb, t.dtype, tuple(t.shape)))
            off += n
        work, res_bytes = [], 0                            # the kernel's item descriptors, and where each result goes
        jitter = []                                        # INPUT.COLOR_JITTER: (offset in the result, h, w, parameters, bgr) of the images that drew any
        for i, k, o, nb, dt, shape in slots:
            if i in recs and k in ("image", "image_trgt"):
                rec = recs[i]
                (newh, neww), (h, w) = rec["size"], shape[:2]
                assert dt == torch.uint8 and len(shape) == 3 and shape[2] == 3, "a DEVICE_RESIZE sample holds a uint8 [h, w, 3] image"
                xt = (slots[tabs[(w, neww)]][2] // 4, rec["xtab"][1]) if neww != w else (-1, 0)
                yt = (slots[tabs[(h, newh)]][2] // 4, rec["ytab"][1]) if newh != h else (-1, 0)
                work.append((o, res_bytes, h, w, newh, neww, int(rec["flip"]), int(rec["reverse_channels"]), *xt, *yt))
                if rec.get("jitter", {}).get(k):
                    jitter.append((res_bytes, newh, neww, rec["jitter"][k], rec["reverse_channels"]))
                res_bytes += (3 * newh * neww + 255) // 256 * 256
        owned = []
        with torch.cuda.stream(self._stream):
            dev = buf[:max(off, 1)].to(self.device, non_blocking=True)
            owned.append(dev)
            if work:
                from . import hip
                res = torch.empty(res_bytes, dtype=torch.uint8, device=self.device)
                hip.resize_batch_u8(dev, res, dev.view(torch.int32) if tabs else None, work)
                if jitter:                                 # (its workspace lives and dies on this stream)
                    hip.color_jitter_batch_u8(res, jitter)
                owned.append(res)
            ev = torch.cuda.Event()
            ev.record(self._stream)
        self._busy.append((ev, buf))
        out = [{k: v for k, v in d.items() if k != DEVICE_RESIZE_KEY} for d in batch]
        fields, done = {}, 0
        for i, k, o, nb, dt, shape in slots:
            if k in ("image", "image_trgt"):
                if i in recs:
                    _, ro, _, _, newh, neww = work[done][:6]
                    out[i][k] = res[ro:ro + 3 * newh * neww].view(3, newh, neww)
                    done += 1
                else:
                    out[i][k] = dev[o:o + nb].view(dt).view(shape)
            elif k in ("gt_boxes", "gt_classes"):
                fields.setdefault(i, {})[k] = dev[o:o + nb].view(dt).view(shape)
        for i, f in fields.items():
            out[i]["instances"] = Instances(batch[i]["instances"].image_size, gt_boxes=Boxes(f["gt_boxes"]), gt_classes=f["gt_classes"])
        return out, ev, owned

    def _run(self):
        import time
        st = self.stats = {"batches": 0, "pull_s": 0.0, "stage_s": 0.0, "handover_wait_s": 0.0}   # where the thread's time goes
        try:
            torch.cuda.set_device(self.device)
            t0 = time.perf_counter()
            for batch in self.batches:
                if self._stop:
                    return
                t1 = time.perf_counter()
                item = self._stage(batch)
                t2 = time.perf_counter()
                self._q.put(item)
                t3 = time.perf_counter()
                st["batches"] += 1; st["pull_s"] += t1 - t0; st["stage_s"] += t2 - t1; st["handover_wait_s"] += t3 - t2
                t0 = t3
                if self._stop:
                    return
            self._q.put(StopIteration())
        except BaseException as e:       # noqa: BLE001 -- handed to the consumer
            self._q.put(e)

    def __next__(self):
        if self._thread is None:
            if self.device.type == "cuda":
                raise StopIteration
            out = []
            for d in next(self.batches):
                d = dict(d)
                for k in ("image", "image_trgt"):
                    if k in d:
                        d[k] = d[k].to(self.device)
                if "instances" in d:
                    d["instances"] = d["instances"].to(self.device)
                out.append(d)
            return out
        item = self._q.get()
        if isinstance(item, BaseException):
            self._thread = None
            if isinstance(item, StopIteration):
                raise StopIteration
            raise item
        out, ev, owned = item
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(ev)
        for t in owned:
            t.record_stream(cur)         # allocated on the staging stream, consumed on the caller's
        return out


def _check_device_resize(cfg, device):
    if cfg.DATALOADER.get("DEVICE_RESIZE", False) and torch.device(device).type != "cuda":
        raise ValueError(f"DATALOADER.DEVICE_RESIZE resizes in a HIP kernel: the loader's device must be a GPU, not {device!r} (there is no host path behind the switch)")


def build_detection_train_loader(cfg, dicts, per_rank_batch, rank=0, world=1, device="cuda", num_workers=None):
    """data/build.py:262-308: mapped infinite stream -> aspect-ratio batches -> device"""
    _check_device_resize(cfg, device)
    mapper = DatasetMapper(cfg, True, np.random.RandomState(cfg.SEED + rank if cfg.SEED >= 0 else None))
    sampler = TrainingSampler(len(dicts), True, max(cfg.SEED, 0), rank, world)
    nw = cfg.DATALOADER.NUM_WORKERS if num_workers is None else num_workers
    ds = _Mapped(dicts, mapper, sampler)
    # workers are SPAWNED, not forked: a forked child of a process that holds a HIP context inherits it (and counts as a GPU process)
    stream = torch.utils.data.DataLoader(ds, batch_size=None, num_workers=nw, prefetch_factor=4, multiprocessing_context="spawn", worker_init_fn=_worker_init) if nw else ds
    # upper bound of a batch's bytes: image + twin, short edge <= max(MIN_SIZE_TRAIN), long edge <= MAX_SIZE_TRAIN
    cap = per_rank_batch * 2 * 3 * (max(cfg.INPUT.MIN_SIZE_TRAIN) or cfg.INPUT.MAX_SIZE_TRAIN) * cfg.INPUT.MAX_SIZE_TRAIN + (per_rank_batch << 16)
    if mapper.device_resize:
        # the ORIGINALS are uploaded (larger than the resized images where the dataset is downscaled), plus a few tables: sized from
        # the dataset's own image sizes; a batch beyond it makes the pinned pool grow
        cap = per_rank_batch * (2 * 3 * max((d.get("height", 0) * d.get("width", 0) for d in dicts), default=0) + (1 << 17))
    return DeviceBatches(aspect_ratio_batches(stream, per_rank_batch), device, max_batch_bytes=cap)


def build_detection_test_loader(cfg, dicts, batch_size=1, rank=0, world=1, device="cuda"):
    """data/build.py:311-357: in order, sharded over ranks (InferenceSampler), annotations dropped by the mapper"""
    _check_device_resize(cfg, device)
    mapper = DatasetMapper(cfg, False)
    n = len(dicts)
    shard = (n + world - 1) // world
    mine = list(range(rank * shard, min((rank + 1) * shard, n)))
    batches = ([mapper(dicts[i]) for i in mine[s:s + batch_size]] for s in range(0, len(mine), batch_size))
    return DeviceBatches(batches, device)
