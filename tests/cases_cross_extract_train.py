"""Training cases of ``embedding_extraction="cross_attention"`` (EmbeddingTransformer.forward in train mode, prompt_encoder.py:289-313).

tools/make_golden_cross_extract_train.py runs the reference's training step (focal objective, class weighting) on the episodes of
tests/cases_cross_extract.py, with the host generator seeded to ``keep_seed`` right before the extraction module draws its query
dropout, and writes tests/golden/cross_extract_<case>_train.{safetensors,json} and cross_extract_<case>_train_logits.safetensors (the train-mode logits in a
file of their own: with the six D / 2 x D projection gradients of the D = 256 case one file would pass the size limit of a committed
file); tests/test_cross_extract_train_*.py read them.
``keep_seed``: seed 0 keeps [T, T, F, F] of the four queries of ``x4``, seed 1 keeps [T, T, T, T, F] of the five of ``x5_d64`` - each mask
drops a query and keeps one, which the generator checks.
"""
XE_TRAIN = [dict(case="x4", seed_gt=17, keep_seed=0), dict(case="x5_d64", seed_gt=17, keep_seed=1)]

EX = "prompt_encoder.embedding_extraction."
_CA = "layers.{l}.cross_attn_image_to_token.{p}_proj.weight"

# gradients stored in full: the small extraction tensors - the learned queries and the three projections the folded kernels stand for
# (q_proj through la_extract_fold_bwd's dq, k_proj through its dW_k, v_proj through la_extract_unfold_bwd) - the last LayerNorm of the
# module, and two tensors upstream of the stream that receive gradient only through la_extract_pool_bwd's dx
XE_TRAIN_FULL = ([EX + "embeddings.weight"] + [EX + _CA.format(l=l, p=p) for l in range(2) for p in "qkv"] +
                 [EX + "layers.1.norm2.weight", "prompt_encoder.transformer.layers.1.norm4.bias", "prompt_encoder.not_a_mask_embed.weight"])

# the 2048-wide MLP weights of both layers: the first rows only (``sliced`` in the fixture's json)
XE_TRAIN_SLICED = [EX + f"layers.{l}.mlp.lin{i}.weight" for l in range(2) for i in (1, 2)]
XE_TRAIN_SLICED_ROWS = 8

# the generator's conditions, recorded in the json: tensors whose gradient norm must lie above the comparison floor (1e-2 of the largest
# norm) - otherwise tests.model_checks.compare_gradients would compare them against the floor, not against themselves
XE_FLOOR = 1e-2
XE_MUST_BE_ABOVE = [EX + "embeddings.weight"] + [EX + _CA.format(l=l, p=p) for l in range(2) for p in "qkv"]
XE_MIN_LIVE_EXTRACTION_ABOVE = 29        # of the 33 live extraction tensors (37 - the four norm3)
# prompt-encoder tensors upstream of the extraction - they see the loss through dx only: case -> (live tensors, how many of them must lie
# above the floor).  x4: 80 of 101 (the reference gives 81).  x5_d64 has box prompts, so point_embeddings.2 / .3 are live too: 103, of which
# the reference puts 76 above the floor (all four point_embeddings, three mask_downscaling tensors, two of sparse_embedding_attention and
# eighteen of the prompt transformer's lie below it under this episode); the condition there is 7 in 10, 72
XE_MIN_UPSTREAM_ABOVE = {"x4": (101, 80), "x5_d64": (103, 72)}
XE_GRAD_TOL = 3e-4                       # the project's GRAD_TOL; the generator asks 4 e_ref32 <= this
