"""Case tables of the text-tower and caption-decoder exact suite (tests/test_gpu_text_exact.py), and the host-side restatement of the
dispatch arithmetic the tables are aimed at.  Imports without a GPU; tests/test_text_bound_host.py asserts that every named class
has a case."""

# ------------------------------------------------------------------------------------------------ skinny GEMM (csrc/gpt2.hip)
SK_MAXM = 64


def skinny_splits(N, K):
    """the fixed K split of an (N, K) shape: enough workgroups for 256 CUs, never more splits than 64-element chunks"""
    tiles, nch = (N + 31) // 32, K // 64
    S = (256 + tiles - 1) // tiles
    return min(S, nch)


def chunks_per_split(N, K):
    S, nch = skinny_splits(N, K), K // 64
    return [nch * (s + 1) // S - nch * s // S for s in range(S)]


def wave_loop(chunks):
    """per wave 0..3 of a workgroup with ``chunks`` chunks: (passes of the two-chunk loop, 1 if a single chunk is left after it),
    following tile_dot's ``for (; c + 4 < c1; c += 8)`` and ``if (c < c1)``"""
    out = []
    for w in range(4):
        c, pairs = w, 0
        while c + 4 < chunks:
            pairs, c = pairs + 1, c + 8
        out.append((pairs, 1 if c < chunks else 0))
    return out


def wave_classes(N, K):
    """the set of chunks-per-wave counts (2 pairs + tail) that some wave of some workgroup of the shape runs"""
    return {2 * p + t for n in set(chunks_per_split(N, K)) for p, t in wave_loop(n)}


# (N, K), chunks per split, what the waves run
SKINNY_SHAPES = [
    ((8, 64), 1, "one chunk: wave 0 the tail, waves 1..3 nothing; one partial tile"),
    ((40, 128), 1, "one chunk per split, two splits, N % 32 = 8"),
    ((768, 3072), 5, "one pair on wave 0 only (4 and 5 chunks per split)"),
    ((8192, 576), 9, "pair + tail on wave 0, one pair on the others"),
    ((8192, 832), 13, "two pairs on wave 0, pair + tail on the others"),
    ((8192, 1024), 16, "two pairs on every wave"),
    ((8192, 1088), 17, "two pairs + tail on wave 0"),
    ((8200, 576), 9, "N with a partial last tile (8 columns) at pair + tail"),
]
SKINNY_M = [1, 32, 33, 64]          # one row; a full row tile; the second row tile with one row; both full
SKINNY_EPI = [0, 1, 2]


def check_skinny_table():
    for (N, K), chunks, _ in SKINNY_SHAPES:
        assert N % 8 == 0 and K % 64 == 0 and max(chunks_per_split(N, K)) == chunks, (N, K, chunks_per_split(N, K))
    classes = set().union(*[wave_classes(N, K) for (N, K), _, _ in SKINNY_SHAPES])
    assert {1, 2, 3, 4, 5} <= classes, classes
    loops = {lp for (N, K), _, _ in SKINNY_SHAPES for n in set(chunks_per_split(N, K)) for lp in wave_loop(n)}
    assert {(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)} <= loops, loops
    assert any(N % 32 for (N, K), _, _ in SKINNY_SHAPES if max(chunks_per_split(N, K)) >= 9)
    assert {1, 32, 33, 64} == set(SKINNY_M) and max(SKINNY_M) == SK_MAXM
    # the shapes of tests/test_gpu_caption.py never pass the two-chunk loop twice and never run pair + tail
    old = set().union(*[wave_classes(N, K) for K, N in [(768, 2304), (768, 768), (768, 3072), (3072, 768), (192, 200)]])
    assert old <= {0, 1, 2}, old


# ------------------------------------------------------------------------------------------------ LM head
LM_V = [5, 32, 33]                   # below one 32-column tile, exactly one, one column into the second
LM_K = 64
LM_B = [1, 5]

# ------------------------------------------------------------------------------------------------ decode attention
DECODE_HEADS = [1, 3]
DECODE_L = {48: [1, 47, 48], 1024: [31, 32, 33, 255, 256, 257]}       # Lmax -> L: the 32 key groups and the 256-thread score loop wrap
BEAM_B, BEAM_P = 5, [0, 1]


def check_decode_table():
    assert set(DECODE_HEADS) == {1, 3}
    assert DECODE_L[48] == [1, 47, 48] and {31, 32, 33, 255, 256, 257} <= set(DECODE_L[1024])
    assert all(L <= Lmax for Lmax, Ls in DECODE_L.items() for L in Ls)


# ------------------------------------------------------------------------------------------------ causal attention (csrc/text_encoder.hip)
ATTN_T = [1, 31, 32, 33, 96, 97, 128]                                   # n = 2, heads = 3
ATTN_WAVES = [(1, 1), (1, 2), (3, 1), (1, 3), (3, 2), (3, 3)]            # (heads, nseq): nseq * heads mod 4 = 1, 2, 3, 3, 2, 1
ATTN_SCALES = [0.125, 0.2]
ATTN_PITCH_PAD = 8                                                      # ldqkv = 3 W + 8, ldo = W + 8


def check_attn_table():
    assert {h * n % 4 for h, n in ATTN_WAVES} == {1, 2, 3} and {h for h, _ in ATTN_WAVES} == {1, 3}
    assert {(t + 31) // 32 for t in ATTN_T} == {1, 2, 3, 4} and {1, 31, 32, 33, 96, 97, 128} == set(ATTN_T)
    assert len(set(ATTN_SCALES)) == 2 and ATTN_PITCH_PAD % 8 == 0


# ------------------------------------------------------------------------------------------------ text_pool, activations, embeddings
POOL_W = [64, 640, 1024]             # W / 64 = 1, 10, 16 registers per lane (16 = POOL_MAXK)
POOL_NOUT = [1, 5]                   # one wave of a block live; a second, partial block
POOL_GROUP = [1, 3, 8]
ACT_NUMEL = {"bf16": [8, 8 * 257], "f32": [4, 4 * 257]}                  # one 16-byte chunk; a partial second block of 256 threads
EMBED_LD_IDS = [1, 9]
EMBED_W = [8, 64]


def check_small_tables():
    assert {w // 64 for w in POOL_W} == {1, 10, 16} and set(POOL_NOUT) == {1, 5} and set(POOL_GROUP) == {1, 3, 8}
    assert all(n // 8 in (1, 257) for n in ACT_NUMEL["bf16"]) and all(n // 4 in (1, 257) for n in ACT_NUMEL["f32"])
    assert set(LM_V) == {5, 32, 33} and set(LM_B) == {1, 5} and LM_K == 64
    assert set(EMBED_LD_IDS) == {1, 9} and 8 in EMBED_W
