#!/usr/bin/env python
"""Golden vectors of ``embedding_extraction="cross_attention"`` from the REFERENCE (build container only; tools/golden_lib.py
imports it):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_cross_extract.py [--only NAME]

For every case of tests/cases_cross_extract.py the seeded weights (``init_state_dict``: the 37 added tensors come last) are strict-loaded
into ``_build_lam(..., embedding_extraction="cross_attention")`` and the seeded episode runs through the reference's ``Lam.forward`` on
CPU / fp32.  tests/golden/cross_extract_<case>.safetensors holds the reference's OUTPUTS: class_examples_embeddings, the returned
flag_examples, low_res_logits, logits and argmax.  cross_extract_<case>_stream.safetensors holds every ``stream_stride``-th row and column
of the stream handed to the extraction module together with what the reference's module returns for exactly those rows
(``sub_embeddings``), the operands of the torch restatement in tests/cross_extract_ref.py.  The json lists the 37 added key names and, per
layer, the smallest and largest score spread (max - min along the keys) over all attention rows of the full forward; the generator
refuses a fixture in which some row's spread is below the case's ``min_spread`` (1.5; 0.5 for the heads of width 4 of the D = 64 case, see
tests/cases_cross_extract.py) or the largest below 5 - a near-uniform softmax would hide a wrong softmax.
"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tools.golden_lib as GL          # noqa: E402  (makes the reference importable)

import torch                            # noqa: E402
from tests.cases_cross_extract import XE_CASES   # noqa: E402

PRE = "prompt_encoder.embedding_extraction."
MAX_SPREAD = 5.0


def run(name, case):
    cfg = case["cfg"]
    lam, sd, batch, rows = GL.reference_episode(
        case, embedding_extraction="cross_attention",
        # handed over UNRESOLVED where the case is segment_example_logits alone, so that the reference's own builder resolves them
        segment_example_logits=cfg.segment_example_logits,
        embeddings_per_example=cfg.embeddings_per_example if cfg.embeddings_per_example > 1 else None)
    b, m, c = batch["flag_examples"].shape
    module = lam.prompt_encoder.embedding_extraction
    seen = {}
    spreads = [[], []]

    def grab(mod, args):
        seen["src"], seen["image_pe"], seen["flags"] = args[0].detach().clone(), args[1], args[2]

    def spread_of(layer):
        def hook(mod, args, kwargs):
            q, k = kwargs["q"], kwargs["k"]
            heads = mod.num_heads
            qh = mod._separate_heads(mod.q_proj(q), heads)
            kh = mod._separate_heads(mod.k_proj(k), heads)
            s = qh @ kh.permute(0, 1, 3, 2) / math.sqrt(qh.shape[-1])
            spreads[layer].append((s.max(-1).values - s.min(-1).values).flatten())
        return hook

    handles = [module.register_forward_pre_hook(grab)]
    handles += [module.layers[l].cross_attn_image_to_token.register_forward_pre_hook(spread_of(l), with_kwargs=True) for l in range(2)]
    with torch.no_grad():
        seg_low, pe_result = lam._forward(batch)
        for l in range(2):
            spreads[l] = spreads[l][:1]               # (one forward is enough)
        for h in handles[1:]:
            h.remove()
        ref = lam(batch)
        handles[0].remove()
        # the module alone on every stride-th row and column of its stream, with the real flags and with all-ones flags
        st = case["stream_stride"]
        sub = seen["src"][:, :, ::st, ::st].contiguous()
        out_sub = module(sub, seen["image_pe"], seen["flags"])
        out_ones = module(sub, seen["image_pe"], torch.ones_like(seen["flags"]))
    cee = ref["class_examples_embeddings"]
    n = cfg.embeddings_per_example
    assert tuple(cee.shape) == (b, n, c, cfg.embed_dim), cee.shape
    assert "class_embeddings" not in pe_result
    flags = pe_result["flag_examples"]
    assert tuple(flags.shape) == (b, n, c)
    sub_key = next(k for k in out_sub if k != "flag_examples")
    sub_emb = out_sub[sub_key]
    mask_noop = bool(torch.equal(sub_emb, out_ones[sub_key]))
    assert mask_noop, "the key mask changed the module's output"
    stats = [{"min": float(spreads[l][0].min()), "max": float(spreads[l][0].max()), "rows": int(spreads[l][0].numel())} for l in range(2)]
    for l, s in enumerate(stats):
        assert s["min"] >= case["min_spread"] and s["max"] >= MAX_SPREAD, f"[{name}] layer {l}: score spread {s} misses the fixture condition"
    tensors = {
        "class_examples_embeddings": cee.contiguous(),
        "flag_examples": flags.to(torch.uint8).contiguous(),
        **GL.logit_tensors(seg_low, ref),
    }
    # NHWC rows, as the engine holds the stream: (B M C, h' w', D)
    stream = sub.flatten(2).transpose(1, 2).contiguous()
    stream_size = GL.write_fixture(f"cross_extract_{name}_stream", {"stream": stream, "sub_embeddings": sub_emb.contiguous(),
                                                                    "flag_examples_in": seen["flags"].to(torch.uint8).contiguous()}, None)
    added = [k for k in sd if k.startswith(PRE)]
    assert len(added) == 37 and list(sd)[-37:] == added
    meta = {"case": name, "weight_seed": case["weight_seed"], "episode": case["episode"], "queries": int(n), "folded_queries": 8 * int(n),
            "stream_stride": st, "stream_shape": list(stream.shape), "full_stream_shape": list(seen["src"].shape),
            "added_keys": added, "added_shapes": {k: list(sd[k].shape) for k in added}, "score_spread": stats, "min_spread_required": case["min_spread"],
            "key_mask_is_a_no_op": mask_noop, "embedding_scale": float(cee.abs().max()),
            "nan_fraction_of_invalid_classes": float(torch.isnan(ref["logits"]).double().mean())}
    size = GL.write_fixture(f"cross_extract_{name}", tensors, meta, rows)
    print(f"[{name}] n {n} spreads {stats} bytes {size} + {stream_size} scale {meta['embedding_scale']:.3f}")


if __name__ == "__main__":
    GL.main(XE_CASES, run)
