"""Parameter inventory and seeded random initialisation for the hot-path model.

Key names and shapes are the reference's ``Lam.state_dict()`` layout (SURVEY.md
Appendix A; captured from /root/reference/label_anything/models/build_lam.py:96-235,
image_encoder.py, prompt_encoder.py, mask_decoder.py).  HF-ViT keys use the
transformers 4.x names the published checkpoints contain.

Pure CPU torch; used by the product (random-init models for bench / smoke), by
tests and by tools/make_golden.py (so the reference, the oracle and the HIP path
all see bit-identical weights).
"""
from __future__ import annotations

import math
from typing import Dict, List, Tuple

import torch

from .config import LamConfig, EncoderSpec

Shapes = Dict[str, Tuple[int, ...]]


def _attn_shapes(s: Shapes, pre: str, d: int, internal: int) -> None:
    for p in ("q_proj", "k_proj", "v_proj"):
        s[f"{pre}.{p}.weight"] = (internal, d)
        s[f"{pre}.{p}.bias"] = (internal,)
    s[f"{pre}.out_proj.weight"] = (d, internal)
    s[f"{pre}.out_proj.bias"] = (d,)


def _ln_shapes(s: Shapes, pre: str, d: int) -> None:
    s[f"{pre}.weight"] = (d,)
    s[f"{pre}.bias"] = (d,)


def _two_way_shapes(s: Shapes, pre: str, d: int, mlp: int, depth: int = 2) -> None:
    for l in range(depth):
        lp = f"{pre}.layers.{l}"
        _attn_shapes(s, lp + ".self_attn", d, d)
        _attn_shapes(s, lp + ".cross_attn_token_to_image", d, d // 2)
        _attn_shapes(s, lp + ".cross_attn_image_to_token", d, d // 2)
        for n in ("norm1", "norm2", "norm3", "norm4"):
            _ln_shapes(s, f"{lp}.{n}", d)
        s[lp + ".mlp.lin1.weight"] = (mlp, d)
        s[lp + ".mlp.lin1.bias"] = (mlp,)
        s[lp + ".mlp.lin2.weight"] = (d, mlp)
        s[lp + ".mlp.lin2.bias"] = (d,)
    _attn_shapes(s, pre + ".final_attn_token_to_image", d, d // 2)
    _ln_shapes(s, pre + ".norm_final_attn", d)


def _one_way_shapes(s: Shapes, pre: str, d: int, mlp: int, depth: int = 2) -> None:
    """OneWayTransformer = depth x OneWayAttentionBlock (transformer.py:26-66,129-138), in the reference's registration order.  norm3 is
    a parameter of the block that its forward never applies: held, saved and loaded, never read."""
    for l in range(depth):
        lp = f"{pre}.layers.{l}"
        _attn_shapes(s, lp + ".cross_attn_image_to_token", d, d // 2)
        _ln_shapes(s, lp + ".norm1", d)
        s[lp + ".mlp.lin1.weight"] = (mlp, d)
        s[lp + ".mlp.lin1.bias"] = (mlp,)
        s[lp + ".mlp.lin2.weight"] = (d, mlp)
        s[lp + ".mlp.lin2.bias"] = (d,)
        _ln_shapes(s, lp + ".norm2", d)
        _ln_shapes(s, lp + ".norm3", d)


def _attn_mlp_block_shapes(s: Shapes, pre: str, d: int, internal: int, mlp: int) -> None:
    _ln_shapes(s, pre + ".norm", d)
    _attn_shapes(s, pre + ".attn", d, internal)
    s[pre + ".mlp.lin1.weight"] = (mlp, d)
    s[pre + ".mlp.lin1.bias"] = (mlp,)
    s[pre + ".mlp.lin2.weight"] = (d, mlp)
    s[pre + ".mlp.lin2.bias"] = (d,)


def _conv_neck_shapes(s: Shapes, pre: str, cin: int, cout: int) -> None:
    s[pre + ".0.weight"] = (cout, cin, 1, 1)
    _ln_shapes(s, pre + ".1", cout)
    s[pre + ".2.weight"] = (cout, cout, 3, 3)
    _ln_shapes(s, pre + ".3", cout)


def encoder_shapes(spec: EncoderSpec, sam_neck: bool = True, pre: str = "image_encoder") -> Shapes:
    s: Shapes = {}
    e = spec.dim
    if spec.kind == "sam":
        g = spec.img_size // spec.patch
        s[pre + ".pos_embed"] = (1, g, g, e)
        s[pre + ".patch_embed.proj.weight"] = (e, 3, spec.patch, spec.patch)
        s[pre + ".patch_embed.proj.bias"] = (e,)
        for i in range(spec.depth):
            bp = f"{pre}.blocks.{i}"
            _ln_shapes(s, bp + ".norm1", e)
            _ln_shapes(s, bp + ".norm2", e)
            s[bp + ".attn.qkv.weight"] = (3 * e, e)
            s[bp + ".attn.qkv.bias"] = (3 * e,)
            size = g if i in spec.global_idx else spec.window
            s[bp + ".attn.rel_pos_h"] = (2 * size - 1, spec.head_dim)
            s[bp + ".attn.rel_pos_w"] = (2 * size - 1, spec.head_dim)
            s[bp + ".attn.proj.weight"] = (e, e)
            s[bp + ".attn.proj.bias"] = (e,)
            s[bp + ".mlp.lin1.weight"] = (spec.mlp, e)
            s[bp + ".mlp.lin1.bias"] = (spec.mlp,)
            s[bp + ".mlp.lin2.weight"] = (e, spec.mlp)
            s[bp + ".mlp.lin2.bias"] = (e,)
        # the reference always instantiates the SAM neck, even when project_last_hidden=False
        _conv_neck_shapes(s, pre + ".neck", e, spec.out_chans)
    elif spec.kind == "hf":
        s[pre + ".embeddings.cls_token"] = (1, 1, e)
        s[pre + ".embeddings.position_embeddings"] = (1, 1 + spec.pos_grid ** 2, e)
        s[pre + ".embeddings.patch_embeddings.projection.weight"] = (e, 3, spec.patch, spec.patch)
        s[pre + ".embeddings.patch_embeddings.projection.bias"] = (e,)
        for i in range(spec.depth):
            lp = f"{pre}.encoder.layer.{i}"
            _ln_shapes(s, lp + ".layernorm_before", e)
            _ln_shapes(s, lp + ".layernorm_after", e)
            for n in ("query", "key", "value"):
                s[f"{lp}.attention.attention.{n}.weight"] = (e, e)
                s[f"{lp}.attention.attention.{n}.bias"] = (e,)
            s[lp + ".attention.output.dense.weight"] = (e, e)
            s[lp + ".attention.output.dense.bias"] = (e,)
            s[lp + ".intermediate.dense.weight"] = (spec.mlp, e)
            s[lp + ".intermediate.dense.bias"] = (spec.mlp,)
            s[lp + ".output.dense.weight"] = (e, spec.mlp)
            s[lp + ".output.dense.bias"] = (e,)
        _ln_shapes(s, pre + ".layernorm", e)
    elif spec.kind == "dinov3":
        # transformers.DINOv3ViTModel with the ``layer.N.`` spelling of the published checkpoints, in its registration order; mask_token
        # (masked-image pretraining) is held, saved and loaded, never read
        s[pre + ".embeddings.cls_token"] = (1, 1, e)
        s[pre + ".embeddings.mask_token"] = (1, 1, e)
        s[pre + ".embeddings.register_tokens"] = (1, spec.prefix_tokens - 1, e)
        s[pre + ".embeddings.patch_embeddings.weight"] = (e, 3, spec.patch, spec.patch)
        s[pre + ".embeddings.patch_embeddings.bias"] = (e,)
        for i in range(spec.depth):
            lp = f"{pre}.layer.{i}"
            _ln_shapes(s, lp + ".norm1", e)
            s[lp + ".attention.k_proj.weight"] = (e, e)
            if spec.key_bias:
                s[lp + ".attention.k_proj.bias"] = (e,)
            for n in ("v_proj", "q_proj", "o_proj"):
                s[f"{lp}.attention.{n}.weight"] = (e, e)
                s[f"{lp}.attention.{n}.bias"] = (e,)
            s[lp + ".layer_scale1.lambda1"] = (e,)
            _ln_shapes(s, lp + ".norm2", e)
            s[lp + ".mlp.up_proj.weight"] = (spec.mlp, e)
            s[lp + ".mlp.up_proj.bias"] = (spec.mlp,)
            s[lp + ".mlp.down_proj.weight"] = (e, spec.mlp)
            s[lp + ".mlp.down_proj.bias"] = (e,)
            s[lp + ".layer_scale2.lambda1"] = (e,)
        _ln_shapes(s, pre + ".norm", e)
    elif spec.kind == "dinov2":
        # transformers.Dinov2Model in its registration order and spelling; mask_token (masked-image pretraining) is held, never read
        s[pre + ".embeddings.cls_token"] = (1, 1, e)
        s[pre + ".embeddings.mask_token"] = (1, e)
        s[pre + ".embeddings.position_embeddings"] = (1, 1 + spec.pos_grid ** 2, e)
        s[pre + ".embeddings.patch_embeddings.projection.weight"] = (e, 3, spec.patch, spec.patch)
        s[pre + ".embeddings.patch_embeddings.projection.bias"] = (e,)
        for i in range(spec.depth):
            lp = f"{pre}.encoder.layer.{i}"
            _ln_shapes(s, lp + ".norm1", e)
            for n in ("query", "key", "value"):
                s[f"{lp}.attention.attention.{n}.weight"] = (e, e)
                s[f"{lp}.attention.attention.{n}.bias"] = (e,)
            s[lp + ".attention.output.dense.weight"] = (e, e)
            s[lp + ".attention.output.dense.bias"] = (e,)
            s[lp + ".layer_scale1.lambda1"] = (e,)
            _ln_shapes(s, lp + ".norm2", e)
            s[lp + ".mlp.fc1.weight"] = (spec.mlp, e)
            s[lp + ".mlp.fc1.bias"] = (spec.mlp,)
            s[lp + ".mlp.fc2.weight"] = (e, spec.mlp)
            s[lp + ".mlp.fc2.bias"] = (e,)
            s[lp + ".layer_scale2.lambda1"] = (e,)
        _ln_shapes(s, pre + ".layernorm", e)
    else:
        raise ValueError(spec.kind)
    return s


def decoder_shapes(cfg: LamConfig) -> Shapes:
    """neck + prompt_encoder + mask_decoder (everything outside image_encoder.*)."""
    s: Shapes = {}
    d = cfg.embed_dim
    mlp = cfg.dec_mlp
    if cfg.lam_neck:
        _conv_neck_shapes(s, "neck", cfg.image_embed_dim, d)
    pe = "prompt_encoder"
    s[pe + ".pe_layer.positional_encoding_gaussian_matrix"] = (2, d // 2)
    for i in range(4):
        s[f"{pe}.point_embeddings.{i}.weight"] = (1, d)
    for n in ("not_a_point_embed", "no_mask_embed", "no_sparse_embedding", "not_a_mask_embed"):
        s[f"{pe}.{n}.weight"] = (1, d)
    c1, c2 = cfg.mask_in_chans // 4, cfg.mask_in_chans
    s[pe + ".mask_downscaling.0.weight"] = (c1, 1, 2, 2)
    s[pe + ".mask_downscaling.0.bias"] = (c1,)
    _ln_shapes(s, pe + ".mask_downscaling.1", c1)
    s[pe + ".mask_downscaling.3.weight"] = (c2, c1, 2, 2)
    s[pe + ".mask_downscaling.3.bias"] = (c2,)
    _ln_shapes(s, pe + ".mask_downscaling.4", c2)
    s[pe + ".mask_downscaling.6.weight"] = (d, c2, 1, 1)
    s[pe + ".mask_downscaling.6.bias"] = (d,)
    _two_way_shapes(s, pe + ".transformer", d, mlp)
    if cfg.bank_size:
        s[pe + ".class_encoder.pos_embedding"] = (1, 1, cfg.bank_size, d)
    _attn_mlp_block_shapes(s, pe + ".sparse_embedding_attention", d, d, mlp)
    if cfg.class_attention:
        _attn_mlp_block_shapes(s, pe + ".class_attention", d, d // 2, mlp)
    if cfg.example_class_attention:
        _attn_mlp_block_shapes(s, pe + ".class_example_attention", d, d // 2, mlp)
    if cfg.example_attention:
        _attn_mlp_block_shapes(s, pe + ".example_attention", d, d // 2, mlp)
    md = "mask_decoder"
    if cfg.one_way:
        _one_way_shapes(s, md + ".transformer", d, mlp)
    else:
        _two_way_shapes(s, md + ".transformer", d, mlp)
    c1, cf = cfg.up_mid, cfg.class_width                          # D // 4 and D // 8 at the default downsample rate of 8
    s[md + ".output_upscaling.0.weight"] = (d, c1, 2, 2)          # ConvTranspose2d: (Cin, Cout, kh, kw)
    s[md + ".output_upscaling.0.bias"] = (c1,)
    _ln_shapes(s, md + ".output_upscaling.1", c1)
    s[md + ".output_upscaling.3.weight"] = (c1, cf, 2, 2)
    s[md + ".output_upscaling.3.bias"] = (cf,)
    s[md + ".class_mlp.layers.0.weight"] = (d, d)
    s[md + ".class_mlp.layers.0.bias"] = (d,)
    s[md + ".class_mlp.layers.1.weight"] = (d, d)
    s[md + ".class_mlp.layers.1.bias"] = (d,)
    s[md + ".class_mlp.layers.2.weight"] = (cf, d)
    s[md + ".class_mlp.layers.2.bias"] = (cf,)
    if cfg.spatial_convs:
        ch = cf
        for i in range(cfg.spatial_convs):
            s[f"{md}.spatial_convs.{3 * i}.weight"] = (ch, ch, 3, 3)
            s[f"{md}.spatial_convs.{3 * i}.bias"] = (ch,)
            if i < cfg.spatial_convs - 1:
                _ln_shapes(s, f"{md}.spatial_convs.{3 * i + 1}", ch)
    if cfg.classification_levels == 2:
        # LAST, so that every other tensor of init_state_dict(cfg, seed) is the one of the classification_levels = 1 model
        s[md + ".level_reducer.weight"] = (1, 2, 3, 3)                # (out, level, ky, kx): level 0 = fine, 1 = enlarged coarse
        s[md + ".level_reducer.bias"] = (1,)
    if cfg.conv_classification:
        # LAST as well (never together with the level reducer): ConvTranspose2d(cf, cf, 3, bias=False) weights, (in, out, ky, kx)
        s[md + ".prototype_tconv.0.weight"] = (cf, cf, 3, 3)
        s[md + ".prototype_tconv.1.weight"] = (cf, cf, 3, 3)
    if cfg.embedding_extraction == "cross_attention":
        # LAST as well: EmbeddingTransformer (prompt_encoder.py:280-287) = 2 x OneWayAttentionBlock (transformer.py:129-138) + the learned
        # queries, 37 tensors.  norm3 is a parameter of the block that its forward never applies: held and saved, never read.
        ex = pe + ".embedding_extraction"
        for l in range(2):
            lp = f"{ex}.layers.{l}"
            _attn_shapes(s, lp + ".cross_attn_image_to_token", d, d // 2)
            for n in ("norm1", "norm2", "norm3"):
                _ln_shapes(s, f"{lp}.{n}", d)
            s[lp + ".mlp.lin1.weight"] = (mlp, d)
            s[lp + ".mlp.lin1.bias"] = (mlp,)
            s[lp + ".mlp.lin2.weight"] = (d, mlp)
            s[lp + ".mlp.lin2.bias"] = (d,)
        s[ex + ".embeddings.weight"] = (int(cfg.embeddings_per_example), d)
    return s


def model_shapes(cfg: LamConfig) -> Shapes:
    s: Shapes = {}
    spec = cfg.encoder_spec
    if spec is not None:
        s.update(encoder_shapes(spec))
    s.update(decoder_shapes(cfg))
    return s


# prototype_tconv.{0,1}: std = 1 / sqrt(9 cf), the fan-in of a 3 x 3 convolution over cf channels.  An entry of the composed 5 x 5 kernel
# sums cf products in the first layer and up to 9 cf in the second, which makes it |e| / 3 at the centre tap and less towards the rim; a
# logit then sums 25 cf products of features and kernel entries.  Measured on the fixtures (tests/golden/convcls_r*.json, "scale"): the
# low-resolution logits have an rms of 3.6 (max 12) at cf = 256 and 1.7 (max 6) at cf = 32, next to 5.4 for the plain dot product.
PROTOTYPE_TCONV_FAN = 9

_NORM_TAGS = (".norm", ".layernorm", "neck.1.", "neck.3.", "mask_downscaling.1.", "mask_downscaling.4.",
              "output_upscaling.1.", "spatial_convs.1.", "spatial_convs.4.", "spatial_convs.7.")


def _is_norm(name: str) -> bool:
    return any(t in name for t in _NORM_TAGS)


def init_state_dict(cfg: LamConfig, seed: int = 0) -> Dict[str, torch.Tensor]:
    """Seeded, fan-in scaled random weights.  Every tensor is non-trivial (rel-pos tables and
    pos_embed are NOT zero-initialised as in the reference, image_encoder.py:72-74,236-237, so
    positional bugs cannot hide)."""
    gen = torch.Generator().manual_seed(seed)
    out: Dict[str, torch.Tensor] = {}
    for name, shape in model_shapes(cfg).items():
        if name.endswith(".lambda1"):
            # LayerScale: uniform on [0.05, 1.5] and not the checkpoints' initial 1.0, so that folding it into a projection is never a no-op
            t = 0.05 + 1.45 * torch.rand(shape, generator=gen)
        elif _is_norm(name):
            if name.endswith(".weight"):
                t = 1.0 + 0.1 * torch.randn(shape, generator=gen)
            else:
                t = 0.05 * torch.randn(shape, generator=gen)
        elif name.endswith(".bias"):
            t = 0.02 * torch.randn(shape, generator=gen)
        elif name.endswith("positional_encoding_gaussian_matrix"):
            t = torch.randn(shape, generator=gen)
        elif "rel_pos" in name:
            t = 0.1 * torch.randn(shape, generator=gen)
        elif name.endswith("pos_embed") or "position_embeddings" in name or "cls_token" in name \
                or "pos_embedding" in name or "register_tokens" in name or "mask_token" in name:
            t = 0.02 * torch.randn(shape, generator=gen)
        elif (len(shape) == 2 and shape[0] == 1) or name.endswith("embedding_extraction.embeddings.weight"):
            t = torch.randn(shape, generator=gen)    # nn.Embedding rows: N(0, 1) per entry
        else:
            if "output_upscaling" in name and len(shape) == 4:
                fan_in = shape[0]                    # ConvTranspose2d (Cin, Cout, k, k), stride == k: one tap per output
            elif "prototype_tconv" in name:
                fan_in = PROTOTYPE_TCONV_FAN * shape[0]
            else:
                fan_in = int(math.prod(shape[1:]))
            t = torch.randn(shape, generator=gen) / math.sqrt(max(fan_in, 1))
        out[name] = t.float().contiguous()
    return out
