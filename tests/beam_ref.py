"""numpy-float32 restatements of the beam-search selection rule (cddmsl_beam_step) for tests/test_beam_host.py and
tests/test_gpu_beam.py.  Per caption, B beams with state sum (f32), len, stop, hist [T] (tokens, -1 past the length) and the cache
ancestry anc [T - 1]:

  step 0   beam j takes the j-th (value, index) pair of the caption's row: sum = value - logZ, len = 1;
  step s   a live beam b offers each of its tokens v: cand_sum = sum_b + (logit - logZ_b), cand_len = len_b + 1, a stopped beam
           offers itself once (cand_sum = sum_b, cand_len = len_b, v = 0); key = cand_sum / float(cand_len); the B candidates with
           the largest key survive, ties to the lower b * V + v; new beam j is the j-th survivor.

All arithmetic is np.float32 in exactly this order (numpy's f32 subtraction, addition and division are IEEE)."""
import numpy as np

F = np.float32


def top_b(logits, B):
    """[rows, V] f32 -> (vals [rows, B] f32, idx [rows, B] int32): the B largest, larger value first, lower index among equal values"""
    order = np.argsort(-logits.astype(np.float64), axis=1, kind="stable")[:, :B]
    return np.take_along_axis(logits, order, 1).astype(F), order.astype(np.int32)


def empty_state(n, B, T):
    return {"sum": np.zeros((n, B), F), "len": np.zeros((n, B), np.int32), "stop": np.zeros((n, B), np.uint8),
            "hist": np.full((n, B, T), -1, np.int32), "anc": np.zeros((n * B, T - 1), np.uint8),
            "src": np.zeros((n, B), np.int32), "next_tok": np.zeros(n * B, np.int64)}


def _candidates(vals, idx, logZ, old, c, B, step):
    """the caption's candidates as (key, b, v, cand_sum, cand_len, source was stopped); vals / idx [rows, k] hold k tokens per row"""
    out = []
    for b in range(B):
        row = c * B + b
        s, l = F(old["sum"][c, b]), int(old["len"][c, b])
        if old["stop"][c, b]:
            out.append((F(s / F(l)), b, 0, s, l, True))
            continue
        for k in range(vals.shape[1]):
            logp = F(F(vals[row, k]) - F(logZ[row]))
            cs = F(s + logp)
            out.append((F(cs / F(l + 1)), b, int(idx[row, k]), cs, l + 1, False))
    return out


def beam_step_ref(vals, idx, logZ, old, new, step, stop_id=None):
    """one step for n captions: returns ``new`` (a state whose prior contents stand for the output buffers') with exactly the
    entries the kernel writes replaced.  ``vals`` / ``idx`` may hold any number of tokens per row (B for the kernel's inputs, V
    for a brute force over the whole vocabulary)."""
    n, B, T = old["hist"].shape
    stop_id = -1 if stop_id is None else stop_id
    out = {k: v.copy() for k, v in new.items()}
    for c in range(n):
        if step == 0:
            win = [(None, 0, int(idx[c, j]), F(F(vals[c, j]) - F(logZ[c])), 1, False) for j in range(B)]
        else:
            cands = _candidates(vals, idx, logZ, old, c, B, step)
            win = sorted(cands, key=lambda t: (-float(t[0]), t[1], t[2]))[:B]
        for j, (_, b, v, cs, cl, was) in enumerate(win):
            stopped = was or v == stop_id
            out["sum"][c, j], out["len"][c, j], out["stop"][c, j], out["src"][c, j] = cs, cl, stopped, b
            out["next_tok"][c * B + j] = stop_id if stopped else v
            out["hist"][c, j, :step] = old["hist"][c, b, :step]
            out["hist"][c, j, step] = -1 if was else v
            if step >= 1:
                out["anc"][c * B + j, :step - 1] = old["anc"][c * B + b, :step - 1]
                out["anc"][c * B + j, step - 1] = b
    return out


def random_state(rs, n, B, T, step, stopped, V, stop_id):
    """a state after ``step`` tokens: ``stopped`` [n, B] bool marks beams that ended (at a random earlier length, with stop_id last)"""
    st = empty_state(n, B, T)
    st["hist"][:, :, :step] = rs.randint(0, V, (n, B, step))
    st["len"][:] = step
    for c in range(n):
        for b in range(B):
            if stopped[c, b]:
                l = rs.randint(1, step + 1)
                st["len"][c, b] = l
                st["hist"][c, b, l - 1] = stop_id
                st["hist"][c, b, l:] = -1
    st["stop"][:] = stopped
    st["sum"][:] = (-rs.rand(n, B) * 3 * st["len"]).astype(F)
    st["anc"][:, :max(step - 1, 0)] = rs.randint(0, B, (n * B, max(step - 1, 0)))
    return st
