#!/usr/bin/env python
"""The uniform mean of several checkpoints' weights (checkpoint averaging, the offline form of MODEL_EMA.MODE uniform):

    python tools/average_checkpoints.py --out avg.pth a.pth b.pth c.pth ...

writes ``{"model": ...}`` whose floating-point tensors are the mean of the listed files' ``model`` tensors, computed on the GPU by
``hip.weight_average``: the first file goes in through its copy form, file number n + 1 with w = 1 / (n + 1), the running mean
``MODEL_EMA.MODE uniform`` keeps during training.  The mean is taken in f32 and stored in the dtype of the first file's tensor.
Integer tensors, and entries that some file lacks, are not averaged: they come from the last file that holds them.  A tensor whose
shape differs between two files is an error that names the key.  The result loads through ``MODEL.WEIGHTS``.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def split_keys(states):
    """-> (keys to average, in the first file's order; {key: tensor} taken as they are).  Averaged: floating point in every file and
    present in every file, one shape (else ValueError naming the key).  The rest comes from the last file that holds the key."""
    averaged = []
    for k, v in states[0].items():
        if all(k in s and torch.is_tensor(s[k]) and s[k].is_floating_point() for s in states):
            for s in states[1:]:
                if tuple(s[k].shape) != tuple(v.shape):
                    raise ValueError(f"{k}: shape {tuple(s[k].shape)} in one file, {tuple(v.shape)} in the first")
            averaged.append(k)
    taken, skip = {}, set(averaged)
    for s in states:
        for k, v in s.items():
            if k not in skip:
                taken[k] = v
    return averaged, taken


def average_states(states, accumulate, device="cpu"):
    """``states``: the files' ``model`` dicts in order -> the averaged dict.  ``accumulate(avgs, tensors, w, copy)`` is
    ``hip.weight_average``: called once per file on lists of f32 tensors on ``device``."""
    from cddmsl_amd.solver import average_weight
    averaged, taken = split_keys(states)
    avgs = [torch.zeros(states[0][k].shape, dtype=torch.float32, device=device) for k in averaged]
    for n, s in enumerate(states):
        tensors = [s[k].to(device=device, dtype=torch.float32).contiguous() for k in averaged]
        if n == 0:
            accumulate(avgs, tensors, 0.0, True)
        else:
            accumulate(avgs, tensors, average_weight("uniform", 0.0, n), False)
    out = {}
    for s in states:                                    # the first file's order, then what only later files hold
        for k in s:
            if k not in out:
                out[k] = None
    for k, a in zip(averaged, avgs):
        out[k] = a.to("cpu", states[0][k].dtype)
    for k, v in taken.items():
        out[k] = v
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("files", nargs="+")
    args = ap.parse_args()
    from cddmsl_amd import hip
    from cddmsl_amd.checkpoint import read_state
    assert torch.cuda.is_available(), "average_checkpoints runs its arithmetic on the GPU (hip.weight_average)"
    states = [read_state(f)["model"] for f in args.files]
    out = average_states(states, hip.weight_average, device="cuda")
    torch.cuda.synchronize()
    torch.save({"model": out}, args.out)
    n_avg = len(split_keys(states)[0])
    print(f"{args.out}: mean of {len(states)} files over {n_avg} tensors, {len(out) - n_avg} taken from the last file that holds them")


if __name__ == "__main__":
    main()
