#!/usr/bin/env python
"""Entry point with the reference's CLI (tools/train_caption_consistency.py:134-179, engine/defaults.py:82-141):

    python tools/train_caption_consistency.py --num-gpus 8 --config-file configs/VOC-Experiments/faster_rcnn_CLIP_R_50_C4.yaml \\
        MODEL.CLIP.TEXT_EMB_PATH voc_20_cls_emb.pth SOLVER.IMS_PER_BATCH 128

One process per GPU (engine/launch.py:67-80): with --num-gpus > 1 this script re-launches itself under
``torch.distributed.run`` (RCCL over xGMI).  Datasets are not available offline, so by default the loader is the seeded synthetic
paired-batch generator; ``--voc-root <VOCdevkit/VOC2007> --dt-data <twin dir>`` switches to the real paired VOC pipeline
(cddmsl_amd/data.py), ``--eval-only --voc-root ...`` runs inference + Pascal VOC AP (cddmsl_amd/evaluation.py),
``--datasets-root DIR`` does the same for the Cityscapes / Foggy Cityscapes splits of the AdverseWeather config (paired training
loader; COCO-style box AP on every known DATASETS.TEST name, ``bdd_100k_val`` from its COCO json included; cddmsl_amd/cityscapes.py,
cddmsl_amd/coco_json.py) and for the VOC family of the VOC config (cddmsl_amd/voc_catalog.py: every VOC-family DATASETS.TRAIN name
chained into one paired loader, Pascal VOC AP on ``voc_2007_test`` / ``Clipart1k_test`` / ``Watercolor_test`` / ``Comic_test`` by name;
``--voc-root`` with ``--dt-data`` keeps precedence), ``TEST.EVAL_PERIOD`` repeats that evaluation during training whenever a test set is given, and
``MODEL.WEIGHTS`` / ``--resume`` / ``MODEL.PRE_TRAINED_RCLIP_PATH`` go through cddmsl_amd/checkpoint.py.
``MODEL_EMA.ENABLED True`` keeps an average of the trainable weights (``MODE ema`` with ``DECAY``, or ``uniform`` from ``START_ITER``) on the
GPU after every step, saves it in every checkpoint and evaluates it behind the training weights (``bbox_EMA`` ... lines; ``MODEL_EMA.EVAL``
plain / averaged / both), with ``--eval-only`` from the ``weight_average`` entry of ``MODEL.WEIGHTS``.
``TEST.PROPOSAL_RECALL True`` adds a ``box_proposals`` line (AR@100 ... ARl@1000 of the RPN proposals) per test set to every
evaluation; ``--eval-only MODEL.META_ARCHITECTURE ProposalNetwork`` evaluates backbone + RPN alone and prints only that line.
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def default_argument_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--config-file", default="", metavar="FILE")
    p.add_argument("--resume", action="store_true")
    p.add_argument("--eval-only", action="store_true")
    p.add_argument("--num-gpus", type=int, default=1)
    p.add_argument("--num-machines", type=int, default=1)
    p.add_argument("--machine-rank", type=int, default=0)
    p.add_argument("--dist-url", default="tcp://127.0.0.1:29511")
    p.add_argument("--max-iter", type=int, default=None, help="stop after this many iterations (default: SOLVER.MAX_ITER)")
    p.add_argument("--height", type=int, default=800)
    p.add_argument("--width", type=int, default=1333)
    p.add_argument("--voc-root", default="", help="VOC devkit year directory (Annotations/, ImageSets/Main/, JPEGImages/) for --eval-only")
    p.add_argument("--voc-split", default="test")
    p.add_argument("--dt-data", default="", help="directory name of the domain-translated twins next to the VOC root (e.g. clipart); "
                                                 "with --voc-root, train on the real paired loader instead of synthetic batches")
    p.add_argument("--voc-year", type=int, default=2007)
    p.add_argument("--datasets-root", default="", metavar="DIR",
                   help="directory holding cityscapes/{leftImg8bit,leftImg8bit_foggy,gtFine} and / or VOC2007, VOC2012, dt_clipart, clipart, "
                        "watercolor, comic (Detectron2's DETECTRON2_DATASETS): a Cityscapes DATASETS.TRAIN[0] or VOC-family DATASETS.TRAIN "
                        "names train on the real paired loader, --eval-only scores every known DATASETS.TEST name")
    p.add_argument("opts", default=None, nargs=argparse.REMAINDER)
    return p


def setup(args):
    from cddmsl_amd.config import get_cfg
    cfg = get_cfg()
    if args.config_file:
        cfg.merge_from_file(args.config_file)
    cfg.merge_from_list(args.opts or [])
    return cfg


def build_eval_hook(tr, cfg, args, rank, world, max_iter):
    """hooks.EvalHook (engine/defaults.py:433-447): with TEST.EVAL_PERIOD > 0 and a test set on disk -- ``--datasets-root`` (every
    known DATASETS.TEST name), or ``--voc-root`` with the ``--voc-split`` split -- all ranks evaluate their shard every EVAL_PERIOD
    iterations and once after the last one; rank 0 prints the usual lines behind "iter N" and keeps the values in ``tr.storage``.
    None otherwise: the synthetic loader has no test set."""
    from cddmsl_amd import evaluation
    period = int(cfg.TEST.get("EVAL_PERIOD", 0))
    if period <= 0:
        return None
    if args.datasets_root and not (args.voc_root and args.dt_data):
        fn = lambda prefix: evaluation.run_eval_only_catalog(tr.model, cfg, args.datasets_root, rank, world, return_results=True, prefix=prefix,
                                                             weight_average=tr.weight_average)
    elif args.voc_root and os.path.exists(os.path.join(args.voc_root, "ImageSets", "Main", args.voc_split + ".txt")):
        name = cfg.DATASETS.TEST[0] if cfg.DATASETS.TEST else "voc_" + args.voc_split
        fn = lambda prefix: {name: evaluation.run_eval_only(tr.model, cfg, args, rank, world, return_results=True, prefix=prefix,
                                                            weight_average=tr.weight_average)}
    else:
        return None
    return evaluation.PeriodicEval(tr, period, fn, max_iter, rank)


def eval_proposal_network(cfg, args, rank, world):
    """--eval-only with MODEL.META_ARCHITECTURE ProposalNetwork: the model alone (the trainer does not take it), a detector
    checkpoint's backbone.* / proposal_generator.* (or the seeded synthetic ones), and box_proposals per test set"""
    from cddmsl_amd import evaluation, synthetic
    from cddmsl_amd.checkpoint import DetectionCheckpointer
    from cddmsl_amd.modeling import build_model
    model = build_model(cfg)
    if not cfg.MODEL.WEIGHTS:
        own = model.state_dict()
        model.load_state_dict({k: v for k, v in synthetic.make_state_dict(0, num_classes=cfg.MODEL.ROI_HEADS.NUM_CLASSES).items() if k in own},
                              strict=False)
    else:
        inc = DetectionCheckpointer(model, cfg.OUTPUT_DIR).load(cfg.MODEL.WEIGHTS)
        if rank == 0:
            print(f"checkpoint: {len(inc.missing_keys)} missing, {len(inc.unexpected_keys)} unexpected, {len(inc.incorrect_shapes)} shape-skipped")
    if args.datasets_root and not args.voc_root:
        return evaluation.run_eval_only_catalog(model, cfg, args.datasets_root, rank, world)
    assert args.voc_root, "--eval-only needs --voc-root (a VOC devkit year directory) or --datasets-root: datasets are not shipped"
    return evaluation.run_eval_only(model, cfg, args, rank, world)


def main(args):
    import torch
    from cddmsl_amd import cityscapes, engine, synthetic, voc_catalog
    rank, world = engine.init_distributed()
    from cddmsl_amd.config import auto_scale_workers
    cfg = auto_scale_workers(setup(args), world)                              # engine/defaults.py:374
    cfg.MODEL.DEVICE = f"cuda:{int(os.environ.get('LOCAL_RANK', '0'))}"
    torch.cuda.set_device(cfg.MODEL.DEVICE)
    per_rank = max(cfg.SOLVER.IMS_PER_BATCH // world, 1)       # data/build.py:287
    if args.eval_only and cfg.MODEL.META_ARCHITECTURE == "ProposalNetwork":
        raise SystemExit(eval_proposal_network(cfg, args, rank, world))
    tr = engine.build_trainer(cfg, per_rank, args.height, args.width, seed=cfg.SEED)
    from cddmsl_amd.checkpoint import DetectionCheckpointer
    ckpt = DetectionCheckpointer(tr.model, cfg.OUTPUT_DIR, optimizer=tr.optimizer, trainer=tr, weight_average=tr.weight_average)
    if not cfg.MODEL.WEIGHTS:       # no checkpoints offline: seeded synthetic weights
        tr.model.load_state_dict(synthetic.make_state_dict(0, num_classes=cfg.MODEL.ROI_HEADS.NUM_CLASSES), strict=False)
        tr.clipcap_model.load_state_dict(synthetic.make_mapper_state_dict(1))
    else:                           # defaults.py:396-413 resume_or_load
        inc = ckpt.resume_or_load(cfg.MODEL.WEIGHTS, resume=args.resume)
        if rank == 0:
            print(f"checkpoint: {len(inc.missing_keys)} missing, {len(inc.unexpected_keys)} unexpected, {len(inc.incorrect_shapes)} shape-skipped")
    rclip = cfg.MODEL.get("PRE_TRAINED_RCLIP_PATH", "")
    if rclip and os.path.exists(rclip):
        ckpt.load_offline_backbone(rclip)                                     # train_loop.py:150-161
    elif rclip and rank == 0:
        print(f"MODEL.PRE_TRAINED_RCLIP_PATH {rclip} not found: the offline (teacher) backbone keeps its loaded / synthetic weights")
    if args.eval_only:              # train_caption_consistency.py:143-152: model.eval(); inference over the test sets
        from cddmsl_amd import evaluation
        if args.datasets_root and not args.voc_root:
            raise SystemExit(evaluation.run_eval_only_catalog(tr.model, cfg, args.datasets_root, rank, world, weight_average=tr.weight_average))
        assert args.voc_root, "--eval-only needs --voc-root (a VOC devkit year directory) or --datasets-root: datasets are not shipped"
        raise SystemExit(evaluation.run_eval_only(tr.model, cfg, args, rank, world, weight_average=tr.weight_average))
    if args.voc_root and args.dt_data:      # real paired data; default: seeded synthetic batches
        from cddmsl_amd import data
        from cddmsl_amd.evaluation import VOC_CLASS_NAMES
        dicts = data.load_voc_instances(args.voc_root, "trainval", VOC_CLASS_NAMES[: cfg.MODEL.ROI_HEADS.NUM_CLASSES], dt_data=args.dt_data)
        tr.data_loader = data.build_detection_train_loader(cfg, dicts, per_rank, rank, world, cfg.MODEL.DEVICE)
        tr._data_loader_iter = iter(tr.data_loader)
    elif args.datasets_root and cfg.DATASETS.TRAIN and any(voc_catalog.is_voc_family(n) for n in cfg.DATASETS.TRAIN):
        from cddmsl_amd import data      # the VOC family (configs/VOC-Experiments): every DATASETS.TRAIN name, chained in the order named
        dicts = voc_catalog.load_train_sets(cfg.DATASETS.TRAIN, args.datasets_root, cfg.DATALOADER.FILTER_EMPTY_ANNOTATIONS)
        tr.data_loader = data.build_detection_train_loader(cfg, dicts, per_rank, rank, world, cfg.MODEL.DEVICE)
        tr._data_loader_iter = iter(tr.data_loader)
    elif args.datasets_root and cfg.DATASETS.TRAIN and cityscapes.is_cityscapes(cfg.DATASETS.TRAIN[0]):
        from cddmsl_amd import data      # Cityscapes + Foggy twins (configs/AdverseWeather-Experiments)
        dicts = cityscapes.load_cityscapes(cfg.DATASETS.TRAIN[0], args.datasets_root, device=cfg.MODEL.DEVICE)
        if cfg.DATALOADER.FILTER_EMPTY_ANNOTATIONS:
            dicts = cityscapes.filter_images_with_only_crowd_annotations(dicts)
        tr.data_loader = data.build_detection_train_loader(cfg, dicts, per_rank, rank, world, cfg.MODEL.DEVICE)
        tr._data_loader_iter = iter(tr.data_loader)
    max_iter = args.max_iter or cfg.SOLVER.MAX_ITER
    period = cfg.SOLVER.get("CHECKPOINT_PERIOD", 0)
    eval_hook = build_eval_hook(tr, cfg, args, rank, world, max_iter)        # hooks.EvalHook: TEST.EVAL_PERIOD, when a test set is given
    for it in range(tr.iter, max_iter):
        tr.run_step()
        if eval_hook is not None:
            eval_hook.after_step(it)
        if rank == 0 and tr.metrics_period and it % tr.metrics_period == 0:
            print(f"iter {it}  " + "  ".join(f"{k}: {v:.4f}" for k, v in sorted(tr.storage.items())), flush=True)
        if rank == 0 and period and (it + 1) % period == 0:                   # hooks.PeriodicCheckpointer
            ckpt.save(f"model_{it:07d}", iteration=it)
    if eval_hook is not None:
        eval_hook.after_train()
    if rank == 0 and period:
        ckpt.save("model_final", iteration=max_iter - 1)


if __name__ == "__main__":
    args = default_argument_parser().parse_args()
    if args.num_gpus > 1 and "RANK" not in os.environ:
        port = args.dist_url.rsplit(":", 1)[-1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes", str(args.num_machines), "--node-rank", str(args.machine_rank),
               "--nproc-per-node", str(args.num_gpus), "--master-addr", "127.0.0.1", "--master-port", port] + sys.argv
        sys.exit(subprocess.call(cmd))
    main(args)
