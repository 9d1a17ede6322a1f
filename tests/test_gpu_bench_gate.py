"""The bench's OWN launch shapes under a numeric gate (reference: engine/train_loop.py:311-383, the step bench.py times).

bench.py runs 16 x 800x1333 images per GPU: RoI GEMMs of M = 1 605 632 rows, 3x3 layers of K = 4608 on 12 544 tiles, split-K
tails, persistent kernel forms, 32 GiB of activations -- shapes no other test reaches (the full-size oracle test is ONE image).
Here the trainer is built exactly as bench.py builds it (same config, seeds, synthetic weights and batch), and

  1. the exact-f32 HIP step (the path pinned to the oracle at full size for B = 1 and to the reference's goldens) records its
     proposals;
  2. the bf16 step -- production dispatch -- runs with those proposals forced in (which teacher-forces every index stage) and
     must stay inside the bf16 bounds of test_gpu_e2e.py on every loss and every gradient tensor;
  3. the bf16 step on its own proposals is what bench.py's first step computes: its losses are compared with the committed
     fixture tests/golden/bench_step0_losses.json, which bench.py --full checks its own first step against as well
     (``losses_gate`` in the bench line) -- so the number the bench prints belongs to the computation gated here;
  4. the same at 32 images per GPU for the fp8 configuration against bf16 (BASELINE.json configs[4]).
"""
import gc
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "bench_step0_losses.json")


def bench_trainer(dtype, batch, replay=None):
    """the trainer bench.py times, with the proposal stage on a tape (tests/test_gpu_e2e.py::ProposalTape)"""
    import bench
    from cddmsl_amd import engine, synthetic
    from test_gpu_e2e import ProposalTape
    cfg = bench.make_cfg(dtype)
    cfg.MODEL.DEVICE = "cuda:0"
    tr = engine.build_trainer(cfg, batch, 800, 1333)
    tr.model.load_state_dict(synthetic.make_state_dict(0), strict=False)
    tr.clipcap_model.load_state_dict(synthetic.make_mapper_state_dict(1))
    tr.iter = 20000
    tr.metrics_period = 0
    return tr, ProposalTape(tr.model.proposal_generator, replay)


def first_step(dtype, batch, replay=None, want_grads=True, pre_steps=0):
    """forward + backward of bench.py's FIRST step (no optimizer update): losses, gradients (CPU f32), recorded proposals.
    ``pre_steps``: forward/backward passes run before it on the same batch and seeds (fp8: scale calibration)."""
    from cddmsl_amd import layers
    layers.FP8_SCALES.buf = None                      # a fresh table of delayed-scaling slots for this model
    torch.cuda.reset_peak_memory_stats()
    tr, tape = bench_trainer(dtype, batch, replay)
    data = next(tr._data_loader_iter)
    gens = (tr.model.proposal_generator.sample_generator, tr.model.roi_heads.sample_generator, tr.model.region_generator)
    states = [g.get_state() for g in gens]
    for it in range(pre_steps + 1):
        for g, s in zip(gens, states):
            g.set_state(s)
        tape.recorded = []
        tr.buckets.zero()
        ld = tr.compute_losses(data)
        sum(ld.values()).backward()
        layers.take_touched()
        layers.FP8_SCALES.roll()
    torch.cuda.synchronize()
    tape.close()
    losses = {k: float(v.detach()) for k, v in ld.items()}
    grads = None
    if want_grads:
        grads = {k: p.grad.detach().float().cpu().clone() for k, p in tr.model.named_parameters() if p.requires_grad and p.grad is not None}
    rec = list(tape.recorded)
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    del tr, tape, ld, data
    gc.collect()
    torch.cuda.empty_cache()
    return losses, grads, rec, peak


def compare_grads(got, ref):
    errs = []
    for k, r in ref.items():
        if float(r.abs().max()) < 1e-7:               # attnpool.k_proj.bias: exactly zero in exact arithmetic
            continue
        e = float((got[k] - r).abs().max() / float(r.abs().max()))
        cos = float(torch.nn.functional.cosine_similarity(got[k].flatten().double(), r.flatten().double(), dim=0))
        errs.append((e, cos, k))
    errs.sort(reverse=True)
    return errs


def test_bench_shapes_bf16_against_exact_f32_with_forced_indices():
    from test_gpu_e2e import BF16_GRAD_COS, BF16_GRAD_REL, BF16_GRAD_REL_HEAD, BF16_LOSS_REL, _proposal_diff
    f32_losses, f32_grads, rec, peak32 = first_step("f32", 16)
    bf_losses, bf_grads, rec_bf, peak16 = first_step("bf16", 16, replay=rec)
    assert set(bf_losses) == set(f32_losses) and set(bf_grads) == set(f32_grads)
    worst_l = max(abs(bf_losses[k] - f32_losses[k]) / max(abs(f32_losses[k]), 1e-6) for k in f32_losses)
    errs = compare_grads(bf_grads, f32_grads)
    n_prop = sum(len(b) for b, _ in rec[0])
    own = _proposal_diff(rec_bf[0], rec[0], atol=1.0)
    print(f"bench shapes (16 x 800x1333), bf16 vs exact f32 with forced indices: worst loss rel {worst_l:.5f}; worst gradient "
          f"{errs[0][0]:.4f} ({errs[0][2]}), lowest cosine {min(e[1] for e in errs):.5f}; peak allocated f32 {peak32:.1f} GiB / bf16 {peak16:.1f} GiB; "
          f"bf16's own proposal list differs from f32's (boxes more than 1 px apart) in {own} of {n_prop} entries")
    print("  f32 losses ", f32_losses)
    print("  bf16 losses", bf_losses)
    print("  largest gradient deviations:", [(round(e, 4), round(c, 5), k) for e, c, k in errs[:8]])
    assert n_prop >= 16 * 1000
    for k in f32_losses:
        assert abs(bf_losses[k] - f32_losses[k]) <= BF16_LOSS_REL * abs(f32_losses[k]) + 1e-5, (k, bf_losses[k], f32_losses[k])
    for e, cos, k in errs:
        assert e <= (BF16_GRAD_REL_HEAD if k.startswith("projector.") else BF16_GRAD_REL), (k, e, cos)
        assert cos >= BF16_GRAD_COS, (k, e, cos)
    # the un-forced bf16 step = bench.py's first step: its losses are the fixture bench.py checks itself against
    own_losses, _, _, _ = first_step("bf16", 16, want_grads=False)
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    with open(os.path.join(ROOT, "gpurun_out", "bench_step0_bf16_b16.json"), "w") as f:
        json.dump(own_losses, f)
    print("  bf16 losses on its own proposals (bench.py step 0)", own_losses)
    fx = json.load(open(FIXTURE))["bf16_b16_800x1333"]
    for k, v in fx.items():
        assert abs(own_losses[k] - v) <= 2e-2 * abs(v) + 1e-3, ("bench step-0 fixture", k, own_losses[k], v)
    for k in f32_losses:                                  # and it is the same computation up to the re-dealt samples
        assert abs(own_losses[k] - bf_losses[k]) <= 0.15 * abs(bf_losses[k]) + 2e-2, (k, own_losses[k], bf_losses[k])


def test_bench_shapes_fp8_against_bf16_with_forced_indices():
    """BASELINE.json configs[4]: 32 images per GPU, e4m3 forward + input-gradient GEMMs under the production rule, against the bf16
    step with the bf16 run's proposals forced in; scales calibrated by one earlier pass (delayed scaling).  Bounds as in
    tests/test_gpu_fp8.py (e4m3: 3 mantissa bits): 6 % + 5e-3 on every loss, gradient cosine >= 0.92."""
    from cddmsl_amd import hip
    bf_losses, bf_grads, rec, peak16 = first_step("bf16", 32)
    hip.PROFILE.enable()
    l8, g8, _, peak8 = first_step("fp8", 32, replay=rec, pre_steps=1)
    used = hip.PROFILE.collect()
    assert used.get("k_conv_fwd256_fp8", {}).get("launches", 0) >= 20, {k: v["launches"] for k, v in used.items() if "fp8" in k}
    worst_l = max(abs(l8[k] - bf_losses[k]) / max(abs(bf_losses[k]), 1e-2) for k in bf_losses)
    errs = sorted((c, e, k) for e, c, k in compare_grads(g8, bf_grads))
    print(f"bench shapes (32 x 800x1333), fp8 vs bf16 with forced indices: worst loss rel {worst_l:.4f}; lowest gradient cosines "
          f"{[(round(c, 4), round(e, 3), k) for c, e, k in errs[:6]]}; peak allocated bf16 {peak16:.1f} GiB / fp8 {peak8:.1f} GiB")
    for k in bf_losses:
        assert abs(l8[k] - bf_losses[k]) <= 6e-2 * abs(bf_losses[k]) + 5e-3, (k, l8[k], bf_losses[k])
    assert errs[0][0] >= 0.92, errs[0]
