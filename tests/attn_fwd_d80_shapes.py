"""Shapes for the D = 80 instantiation of the attention forward kernel (rows
of exactly 80 elements, 5 output d-tiles, a half-zero third k step) and for
its 32-row waves, shared by test_attention_fwd_d80_gpu.py and
test_attention_fwd_d80_cases_cpu.py.  The builders, B and H are those of
attn_fwd_cases.py."""

# (S, Skv, D, causal), families A and B.  (256, 256, 80): two q blocks, and
# in the second one interior, diagonal and skipped kv tiles; ragged S and
# Skv; Skv > S and Skv < S under the causal mask; the same geometry at
# DK = 128; D = 48 pads inside DK = 64.
AB_SHAPES = [
    (256, 256, 80, True),
    (200, 200, 80, True),
    (130, 256, 80, True),
    (256, 130, 80, True),
    (256, 256, 128, True),
    (200, 200, 48, True),
]
# (S, d, causal) through the packed-qkv views
VIEW_SHAPES = [
    (256, 80, True),
    (200, 80, False),
]
# (S, Skv, D, causal, order)
STAIR_SHAPES = [(200, 200, 80, True, order)
                for order in ("asc", "desc", "shuffled")] + \
               [(130, 257, 80, False, order)
                for order in ("asc", "desc", "shuffled")]
# (S, Skv, D, causal, alibi, kv_lens)
RANDOM_SHAPES = [
    (256, 256, 80, True, False, None),
    (130, 200, 80, False, True, (200, 64)),
]
DETERMINISM_SHAPE = (256, 256, 80, True, False, None)
# (S, Skv, D, kv_lens), family B with a poisoned tail: one tail starts
# inside a kv tile, the other on a tile edge; 130 q rows fill both 16-row
# sets of a wave and leave the last wave ragged
TAIL_SHAPE = (130, 200, 80, (65, 128))
