"""Model geometry for the LabelAnything hot path.

Mirrors the reference's constructor surface: ``LabelAnything(**kwargs)``
(/root/reference/label_anything/models/build_lam.py:467-508) and the encoder
registry ``ENCODERS`` (models/build_encoder.py:9-28,144-152).  Pure Python; no
device code.
"""
from __future__ import annotations

from dataclasses import dataclass, field, asdict
import math
from typing import Callable, Dict, Optional, Tuple


@dataclass(frozen=True)
class EncoderSpec:
    """One image-encoder geometry.

    kind "sam": ViTDet backbone with 14x14 windowed + global rel-pos attention
    (models/image_encoder.py).  kind "hf": plain pre-LN ViT with CLS token as in
    transformers.ViTModel (models/build_encoder.py:83-100).  kind "dinov3": transformers.DINOv3ViTModel - no position table, 2-D rotary
    embeddings on q and k of the patch tokens in every block, CLS + register tokens in front, LayerScale on both branches.  kind "dinov2":
    transformers.Dinov2Model - the "hf" stack (CLS token, position table resampled bicubically) with 14 x 14 patches, LayerScale on both
    branches, its own key names and the LayerNorm eps of its config.
    """

    kind: str
    dim: int
    depth: int
    heads: int
    mlp: int
    patch: int = 16
    img_size: int = 1024            # SAM: fixed input side (pos_embed size); HF: pretraining side (pos grid)
    global_idx: Tuple[int, ...] = ()
    window: int = 14
    out_chans: int = 256            # SAM neck output channels
    # kinds "dinov3", "dinov2" (DINOv3ViTConfig: num_register_tokens, rope_theta, layerscale_value, key_bias, layer_norm_eps); every other kind keeps
    # the defaults and never reads them
    prefix_tokens: int = 1          # rows in front of the patch tokens: 1 CLS + the register tokens
    rope_theta: float = 100.0
    layer_scale: bool = False       # LayerScale on the attention and the MLP branch
    key_bias: bool = True           # k_proj carries a bias
    ln_eps: float = 1e-12           # of every LayerNorm of the stack (kinds "dinov3", "dinov2": the other kinds' eps is fixed by their block names)

    @property
    def head_dim(self) -> int:
        return self.dim // self.heads

    @property
    def pos_grid(self) -> int:
        return self.img_size // self.patch


_DINOV3 = dict(prefix_tokens=5, rope_theta=100.0, layer_scale=True, key_bias=False, ln_eps=1e-5)
_DINOV2 = dict(patch=14, img_size=518, layer_scale=True, ln_eps=1e-6)

ENCODER_SPECS: Dict[str, EncoderSpec] = {
    # models/build_encoder.py:9-28 (SAM ViT-B/L/H), _build_vit :43-80
    "vit_b": EncoderSpec("sam", 768, 12, 12, 3072, global_idx=(2, 5, 8, 11)),
    "vit_l": EncoderSpec("sam", 1024, 24, 16, 4096, global_idx=(5, 11, 17, 23)),
    "vit_h": EncoderSpec("sam", 1280, 32, 16, 5120, global_idx=(7, 15, 23, 31)),
    # facebook/vit-mae-base / -large geometry (README.md:147-165, parameters/trainval/coco/mael.yaml:49)
    "vit_b_mae": EncoderSpec("hf", 768, 12, 12, 3072, img_size=224),
    "vit_l_mae": EncoderSpec("hf", 1024, 24, 16, 4096, img_size=224),
    # facebook/dino-vitb8 (models/build_encoder.py:115-117): HF ViT-B with 8x8 patches (use vit_patch_size=8)
    "vit_dino_b8": EncoderSpec("hf", 768, 12, 12, 3072, patch=8, img_size=224),
    # google/vit-base-patch16-224-in21k (models/build_encoder.py:108-112): the plain HF ViT-B geometry
    "vit_b_imagenet_i21k": EncoderSpec("hf", 768, 12, 12, 3072, img_size=224),
    # facebook/dinov3-vit{s,b,l}16-pretrain-* (parameters/trainval/coco/dinov3.yaml trains on ViT-B/16 embeddings at 480 px)
    "vit_s_dinov3": EncoderSpec("dinov3", 384, 12, 6, 1536, img_size=224, **_DINOV3),
    "vit_b_dinov3": EncoderSpec("dinov3", 768, 12, 12, 3072, img_size=224, **_DINOV3),
    "vit_l_dinov3": EncoderSpec("dinov3", 1024, 24, 16, 4096, img_size=224, **_DINOV3),
    # facebook/dinov2-{small,base,large} (parameters/trainval/coco/dinov2.yaml trains on ViT-B/14 embeddings at 224 px); position table 37 x 37
    "vit_s_dinov2": EncoderSpec("dinov2", 384, 12, 6, 1536, **_DINOV2),
    "vit_b_dinov2": EncoderSpec("dinov2", 768, 12, 12, 3072, **_DINOV2),
    "vit_l_dinov2": EncoderSpec("dinov2", 1024, 24, 16, 4096, **_DINOV2),
}


def dinov3_spec_from_hf_config(hf: dict) -> EncoderSpec:
    """EncoderSpec of a HuggingFace ``config.json`` with model_type "dinov3_vit".  What the device path does not build is refused here:
    the gated MLP of the S+ / H+ sizes, another activation than GELU, and projections whose bias layout differs from the published one."""
    if hf.get("model_type") != "dinov3_vit":
        raise ValueError(f"not a DINOv3 ViT config: model_type={hf.get('model_type')!r}")
    if hf.get("use_gated_mlp", False):
        raise NotImplementedError("DINOv3 ViT with use_gated_mlp=True (the S+ and H+ sizes: SwiGLU MLP) is not built; the plain-MLP sizes "
                                  "ViT-S/16, ViT-B/16 and ViT-L/16 are")
    if hf.get("hidden_act", "gelu") != "gelu":
        raise NotImplementedError(f"DINOv3 ViT with hidden_act={hf['hidden_act']!r} is not built: only 'gelu'")
    for name, want in (("query_bias", True), ("value_bias", True), ("proj_bias", True), ("mlp_bias", True)):
        if bool(hf.get(name, want)) != want:
            raise NotImplementedError(f"DINOv3 ViT with {name}={hf[name]!r} is not built: only {want}")
    dim, heads = int(hf["hidden_size"]), int(hf["num_attention_heads"])
    if dim % heads or (dim // heads) % 16:
        raise NotImplementedError(f"DINOv3 ViT head width {dim}/{heads}: la_rope_qk rotates head widths that are multiples of 16")
    return EncoderSpec("dinov3", dim, int(hf["num_hidden_layers"]), heads, int(hf["intermediate_size"]), patch=int(hf.get("patch_size", 16)),
                       img_size=int(hf.get("image_size", 224)), prefix_tokens=1 + int(hf.get("num_register_tokens", 0)),
                       rope_theta=float(hf.get("rope_theta", 100.0)), layer_scale=True, key_bias=bool(hf.get("key_bias", False)),
                       ln_eps=float(hf.get("layer_norm_eps", 1e-5)))


def dinov2_spec_from_hf_config(hf: dict) -> EncoderSpec:
    """EncoderSpec of a HuggingFace ``config.json`` with model_type "dinov2" (Dinov2Config has no intermediate_size: the MLP is
    hidden_size * mlp_ratio wide).  Refused here, by name: the register variant, the SwiGLU MLP of the giant size, another activation than
    GELU, q / k / v without biases, and heads wider than the attention kernels' 128 columns."""
    if hf.get("model_type") == "dinov2_with_registers":
        raise NotImplementedError("model_type 'dinov2_with_registers': the register variant of DINOv2 is not built; the plain 'dinov2' "
                                  "checkpoints (small, base, large) are")
    if hf.get("model_type") != "dinov2":
        raise ValueError(f"not a DINOv2 config: model_type={hf.get('model_type')!r}")
    if hf.get("use_swiglu_ffn", False):
        raise NotImplementedError("DINOv2 with use_swiglu_ffn=True (the giant size: SwiGLU MLP) is not built; the plain-MLP sizes "
                                  "small, base and large are")
    if hf.get("hidden_act", "gelu") != "gelu":
        raise NotImplementedError(f"DINOv2 with hidden_act={hf['hidden_act']!r} is not built: only 'gelu'")
    if not hf.get("qkv_bias", True):
        raise NotImplementedError("DINOv2 with qkv_bias=False is not built: only q / k / v projections with biases")
    dim, heads = int(hf["hidden_size"]), int(hf["num_attention_heads"])
    if dim % heads or dim // heads > 128:
        raise NotImplementedError(f"DINOv2 head width {dim}/{heads}: the attention kernels take heads of at most 128 columns")
    return EncoderSpec("dinov2", dim, int(hf["num_hidden_layers"]), heads, int(dim * hf.get("mlp_ratio", 4)), patch=int(hf.get("patch_size", 14)),
                       img_size=int(hf.get("image_size", 518)), layer_scale=True, ln_eps=float(hf.get("layer_norm_eps", 1e-6)))


def vit_spec_from_hf_config(hf: dict) -> EncoderSpec:
    """EncoderSpec of a HuggingFace ``config.json`` of the plain ViT family (ViTModel, ViTMAEModel): every model_type no other kind claims."""
    return EncoderSpec("hf", dim=hf["hidden_size"], depth=hf["num_hidden_layers"], heads=hf["num_attention_heads"], mlp=hf["intermediate_size"],
                       patch=hf.get("patch_size", 16), img_size=hf.get("image_size", 224))


@dataclass(frozen=True)
class BlockNames:
    """Where one kind of encoder keeps the tensors of a transformer block: ``prefix.format(i)`` + "." + a name below + ".weight" / ".bias"."""
    prefix: str
    norm1: str
    qkv: Tuple[str, ...]          # one fused q | k | v tensor, or q, k, v
    proj: str
    norm2: str
    lin1: str
    lin2: str
    eps: float                    # of every LayerNorm of the stack


SAM_BLOCK = BlockNames("image_encoder.blocks.{}", "norm1", ("attn.qkv",), "attn.proj", "norm2", "mlp.lin1", "mlp.lin2", 1e-6)
HF_BLOCK = BlockNames("image_encoder.encoder.layer.{}", "layernorm_before",
                      ("attention.attention.query", "attention.attention.key", "attention.attention.value"), "attention.output.dense",
                      "layernorm_after", "intermediate.dense", "output.dense", 1e-12)
# DINOv3 ViT (transformers DINOv3ViTLayer).  ``o_ls`` / ``down_ls`` are not checkpoint tensors: LamEngine._fold_layer_scale derives them from
# o_proj / down_proj and the block's LayerScale vectors; eps comes from the spec (EncoderKind.spec_eps).
DINOV3_BLOCK = BlockNames("image_encoder.layer.{}", "norm1", ("attention.q_proj", "attention.k_proj", "attention.v_proj"), "attention.o_ls",
                          "norm2", "mlp.up_proj", "mlp.down_ls", 1e-5)
# DINOv2 (transformers Dinov2Layer): the HF block with its own LayerNorm / MLP names; ``output.ls`` / ``fc2_ls`` are derived like DINOv3's.
DINOV2_BLOCK = BlockNames("image_encoder.encoder.layer.{}", "norm1",
                          ("attention.attention.query", "attention.attention.key", "attention.attention.value"), "attention.output.ls",
                          "norm2", "mlp.fc1", "mlp.fc2_ls", 1e-6)


@dataclass(frozen=True)
class EncoderKind:
    """Everything the code asks about ``EncoderSpec.kind``, as data.  Tensor names are relative to ``image_encoder.``."""
    blocks: BlockNames
    patch: str                                      # the patch embedding: + ".weight" / ".bias"
    final_norm: Optional[str]                       # the LayerNorm behind the block stack (SAM: none, the neck follows)
    builder: str                                    # the function of models.py that builds the encoder-only model
    train_graph: str                                # the class of train_encoder.py that trains the stack, or ...
    train_refusal: Optional[str] = None             # ... why LamTrainer(train_encoder=True) refuses the kind (then train_graph is "")
    default_side: Optional[int] = 480               # input side of ImageEncoder when none is given; None: the spec's img_size
    spec_eps: bool = False                          # LayerNorm eps from spec.ln_eps (else blocks.eps)
    layer_scale: Optional[Tuple[str, str]] = None   # the checkpoint's projections LayerScale folds into: sources of blocks.proj, blocks.lin2
    prefix: Tuple[str, ...] = ()                    # the tensors whose rows stand in front of every image's patch rows
    pos_table: bool = False                         # embeddings.position_embeddings: added to every row, resampled to the input's grid
    rope: bool = False                              # q and k of the patch rows are rotated in every block (la_rope_qk)
    square: Optional[str] = None                    # the family's name where inputs must be square
    mask_token: bool = False                        # the checkpoint's mask_token is a parameter of the encoder (else of a decoder: dropped)
    imagenet_stats: bool = False                    # embeddings are made with the ImageNet mean / std whatever the caller asks for
    model_types: Tuple[str, ...] = ()               # HuggingFace ``model_type`` values the kind claims (spec_from_hf refuses what is not built)
    spec_from_hf: Optional[Callable[[dict], EncoderSpec]] = None


_HF_PATCH, _CLS, _FROZEN = "embeddings.patch_embeddings.projection", "embeddings.cls_token", "embeddings (use_vit=False) or keep the encoder frozen"
ENCODER_KINDS: Dict[str, EncoderKind] = {
    "sam": EncoderKind(SAM_BLOCK, "patch_embed.proj", None, "_build_sam_encoder", "SamEncoderGraph", default_side=None),
    "hf": EncoderKind(HF_BLOCK, _HF_PATCH, "layernorm", "_build_hf_encoder", "HfEncoderGraph", prefix=(_CLS,), pos_table=True,
                      spec_from_hf=vit_spec_from_hf_config),
    "dinov2": EncoderKind(DINOV2_BLOCK, _HF_PATCH, "layernorm", "_build_hf_encoder", "", spec_eps=True,
                          layer_scale=("attention.output.dense", "mlp.fc2"), prefix=(_CLS,), pos_table=True, square="DINOv2", mask_token=True,
                          imagenet_stats=True, model_types=("dinov2", "dinov2_with_registers"), spec_from_hf=dinov2_spec_from_hf_config,
                          train_refusal="train_encoder=True with a 'dinov2' encoder is not built: the gradients of LayerScale and of the "
                                        "padded patch embedding (la_im2col_patch_pad's operand) do not exist; train on precomputed " + _FROZEN),
    "dinov3": EncoderKind(DINOV3_BLOCK, "embeddings.patch_embeddings", "norm", "_build_hf_encoder", "", spec_eps=True,
                          layer_scale=("attention.o_proj", "mlp.down_proj"), prefix=(_CLS, "embeddings.register_tokens"), rope=True,
                          square="DINOv3", mask_token=True, imagenet_stats=True, model_types=("dinov3_vit",),
                          spec_from_hf=dinov3_spec_from_hf_config,
                          train_refusal="train_encoder=True with a 'dinov3' encoder is not built: the backward of la_rope_qk (the inverse "
                                        "rotation) and the gradients of LayerScale and the register tokens do not exist; train on "
                                        "precomputed " + _FROZEN),
}


def encoder_kind(kind: str) -> EncoderKind:
    """The one lookup of an encoder kind: everything that depends on ``EncoderSpec.kind`` reads the record it returns."""
    try:
        return ENCODER_KINDS[kind]
    except KeyError:
        raise ValueError(f"no encoder driver for kind {kind!r}; known kinds: {sorted(ENCODER_KINDS)}") from None


def spec_from_hf_config(hf: dict) -> EncoderSpec:
    """EncoderSpec of a HuggingFace ``config.json``: by the kind that claims its model_type, the plain ViT family otherwise."""
    for rec in ENCODER_KINDS.values():
        if hf.get("model_type") in rec.model_types:
            return rec.spec_from_hf(hf)
    return vit_spec_from_hf_config(hf)


def register_encoder(name: str, spec: EncoderSpec) -> None:
    """Register an extra geometry (used by tests for reduced-size encoders)."""
    ENCODER_SPECS[name] = spec


@dataclass
class LamConfig:
    """Keyword surface of ``LabelAnything.__init__`` (build_lam.py:470-498), on-path subset.

    Off-path switches (few_type=Affinity, Identity fusion, binary, pyramids,
    class_embedding_dim) are accepted only at their default value; anything else raises NotImplementedError.
    ``fusion_transformer`` takes "TwoWayTransformer" and, for models without an image encoder, "OneWayTransformer".
    ``embedding_extraction`` takes None and "cross_attention"; every other value ("pooler" ...) raises NotImplementedError.
    """

    encoder: Optional[str] = "vit_b"
    use_vit: bool = True
    use_vit_sam_neck: bool = True
    image_embed_dim: int = 256
    embed_dim: int = 256
    image_size: int = 1024
    vit_patch_size: int = 16
    class_attention: bool = False
    example_attention: bool = False
    example_class_attention: bool = True
    spatial_convs: Optional[int] = None
    class_encoder: Optional[dict] = None      # {"name": "RandomMatrixEncoder", "bank_size": 100, "embed_dim": D}
    custom_preprocess: bool = True
    # Dropout probability of the decoder-side MLP / attention blocks (models/common.py:25-32,68-75, build_lam.py:128).  An inference
    # no-op (eval mode); remembered so that LamTrainer can refuse to train a configuration whose reference applies it.
    dropout: float = 0.0
    # Per-example family (build_lam.py:126,145-148): k x k pooled embeddings per (support, class) go through the mask decoder as tokens and
    # every pixel takes the maximum over the valid examples of a class (prompt_encoder.py:726-731, mask_decoder.py:279-287,299-314).
    # Stored RESOLVED (resolve_examples): segment_example_logits alone means one embedding per example, any truthy
    # embeddings_per_example turns segment_example_logits on.  Adds no parameters.
    segment_example_logits: bool = False
    embeddings_per_example: Optional[int] = None
    # 2: the decoder owns level_reducer = Conv2d(2, 1, 3x3, "same") over [fine logits, x4 enlargement of the transformer-level logits]
    # (mask_decoder.py:204,345-346,358-362; parameters/trainval/pascal/mae_levels.yaml).  The reference's forward stacks exactly two
    # levels, so 1 and 2 are the values that can run.  Adds mask_decoder.level_reducer.{weight,bias}.
    classification_levels: int = 1
    # Channel widths of the mask decoder's upscaler (mask_decoder.py:198-255): output_upscaling.0 gives embed_dim // max(r // 2, 1)
    # channels, output_upscaling.3, class_mlp's last layer and the spatial convolutions embed_dim // r.  1 and 8 are built
    # (parameters/trainval/pascal/mae_nodown.yaml uses 1).
    classification_layer_downsample_rate: int = 8
    # True: the decoder owns prototype_tconv = 2 x ConvTranspose2d(cf, cf, 3, bias=False), which turn every prototype into a cf x 5 x 5
    # kernel; the logits are the 5 x 5 cross-correlation of the feature map with it (mask_decoder.py:257-271,299-307).  Adds
    # mask_decoder.prototype_tconv.{0,1}.weight.
    conv_classification: bool = False
    # "cross_attention": the per-example embeddings are not pooled from the stream but read out of it by ``embeddings_per_example`` learned
    # queries through two OneWayAttentionBlocks over the M hw rows of every (episode, class) pair (EmbeddingTransformer,
    # prompt_encoder.py:280-313,719-724; parameters/validation/Pascal/mae_cross.yaml).  Adds 37 tensors under
    # prompt_encoder.embedding_extraction.; the three merge attentions are not run.  embeddings_per_example need not be a square.
    embedding_extraction: Optional[str] = None
    # "TokenPool": PromptImagePoolEncoder (prompt_encoder.py:830-915; parameters/trainval/{pascal,coco20i}/mae_pool.yaml).  The dense
    # prompts of a support's C classes are summed into ONE slab per support image, the two-way transformer runs over B M slabs with the
    # C Ns tokens of the support, and an example's embedding is the mean of its class's OUTPUT tokens - so final_attn_token_to_image and
    # norm_final_attn, dead in the plain prompt encoder, are live.  Adds no parameters.
    prompt_encoder: Optional[str] = None
    # "OneWayTransformer": the mask decoder's transformer (and only it: the prompt encoder's two-way transformer is hard-wired,
    # build_lam.py:198-205,238-275) leaves the class tokens as they are and runs, per layer, image -> token cross attention + norm1 and a
    # dec_mlp-wide ReLU MLP + norm2 on EVERY pixel row (transformer.py:26-154; parameters/trainval/Ablations/mae_transformer.yaml).
    # mask_decoder.transformer.* is then 36 tensors; norm3 of a block is a parameter its forward never applies.  Built for models
    # without an image encoder (use_vit=False), which is what every reference recipe with this switch builds.
    fusion_transformer: str = "TwoWayTransformer"
    # fixed in the reference for this path
    dec_heads: int = 8
    dec_mlp: int = 2048
    mask_in_chans: int = 16

    @property
    def grid(self) -> int:
        return self.image_size // self.vit_patch_size

    @property
    def lam_neck(self) -> bool:
        return self.image_embed_dim != self.embed_dim

    @property
    def up_mid(self) -> int:
        """Channels after output_upscaling.0 (mask_decoder.py:198-202,210)."""
        return self.embed_dim // max(self.classification_layer_downsample_rate // 2, 1)

    @property
    def class_width(self) -> int:
        """Channels of the map the pixels are classified on, = the prototype width (mask_decoder.py:218,226)."""
        return self.embed_dim // self.classification_layer_downsample_rate

    @property
    def encoder_spec(self) -> Optional[EncoderSpec]:
        if not self.use_vit or self.encoder is None:
            return None
        return ENCODER_SPECS[self.encoder]

    @property
    def one_way(self) -> bool:
        return self.fusion_transformer == "OneWayTransformer"

    @property
    def pool_side(self) -> int:
        """k of the k x k adaptive average pool: floor(sqrt(embeddings_per_example)) (prompt_encoder.py:727); 1 = the plain mean."""
        e = self.embeddings_per_example
        if self.embedding_extraction is not None:       # the learned queries replace the pooling (prompt_encoder.py:722-724)
            return 1
        return math.isqrt(int(e)) if e and int(e) > 1 else 1

    @property
    def bank_size(self) -> int:
        return int(self.class_encoder["bank_size"]) if self.class_encoder else 0


_OFF_PATH_DEFAULTS = dict(
    class_embedding_dim=None,
    encoder_attention_downsample_rate=2, decoder_attention_downsample_rate=2,
    use_support_features_in_prompt_encoder=True,
    few_type="Prototype", class_fusion="sum",
    transformer_keys_are_images=True, transformer_feature_size=None,
    dropout=0.0, binary=False,
)


def resolve_examples(segment_example_logits, embeddings_per_example):
    """build_lam.py:145-148 -> (segment_example_logits, embeddings_per_example) as the reference's builder resolves them."""
    seg = bool(segment_example_logits)
    epe = None if embeddings_per_example is None else int(embeddings_per_example)
    if epe is not None and epe < 0:
        raise ValueError(f"embeddings_per_example={epe} must not be negative")
    if seg and epe is None:
        epe = 1
    if epe and not seg:
        seg = True
    return seg, epe


def check_extraction(embedding_extraction, embeddings_per_example, embed_dim: int = 256) -> None:
    """The one check of ``embedding_extraction`` (config_from_kwargs and Lam), on the RESOLVED embeddings_per_example."""
    if embedding_extraction is None:
        return
    if embedding_extraction != "cross_attention":
        raise NotImplementedError(f"embedding_extraction={embedding_extraction!r} is not built: only None and 'cross_attention' "
                                  f"(prompt_encoder.py:442-447; 'pooler' draws Gumbel noise in eval and needs the `masks` loss)")
    if not embeddings_per_example or int(embeddings_per_example) < 1:
        raise ValueError("embedding_extraction='cross_attention' needs embeddings_per_example >= 1 learned queries (the reference "
                         "fails in nn.Embedding(None, D), prompt_encoder.py:286); segment_example_logits alone resolves to 1")
    if int(embeddings_per_example) > 16:
        raise NotImplementedError(f"embeddings_per_example={embeddings_per_example} with embedding_extraction='cross_attention': "
                                  f"la_extract_pool takes up to 16 queries per pair")
    if embed_dim not in (64, 128, 256):
        raise NotImplementedError(f"embedding_extraction='cross_attention' with embed_dim={embed_dim}: la_extract_pool is built for the "
                                  f"widths 64, 128 and 256")


def check_levels(levels, segment_example_logits) -> None:
    """The one check of ``classification_levels`` (config_from_kwargs and Lam): an int, 1 or 2, and 2 not with the per-example family."""
    if isinstance(levels, bool) or not isinstance(levels, int) or levels not in (1, 2):
        raise ValueError(f"classification_levels={levels!r}: the reference's mask decoder stacks exactly two levels (mask_decoder.py:360), "
                         f"so only the integers 1 and 2 can run")
    if levels == 2 and segment_example_logits:
        raise NotImplementedError("classification_levels=2 together with segment_example_logits / embeddings_per_example is not built: the "
                                  "only reference recipe that combines them (parameters/trainval/pascal/mae_chooser.yaml) also needs the "
                                  "`pooler` embedding extraction and the `masks` loss, neither of which is built")


def check_classification(rate, conv_classification, segment_example_logits, levels) -> None:
    """The one check of ``classification_layer_downsample_rate`` and ``conv_classification`` (config_from_kwargs and Lam)."""
    if isinstance(rate, bool) or not isinstance(rate, int) or rate not in (1, 2, 4, 8):
        raise ValueError(f"classification_layer_downsample_rate={rate!r}: a power of two from 1 to 8 (it divides embed_dim twice, "
                         f"mask_decoder.py:198-226)")
    if rate not in (1, 8):
        raise NotImplementedError(f"classification_layer_downsample_rate={rate}: only 1 and 8, the values of the reference's recipes, "
                                  f"are built")
    if conv_classification and segment_example_logits:
        raise NotImplementedError("conv_classification together with segment_example_logits / embeddings_per_example is not built: the "
                                  "reference's _classify groups the N C kernels by C there (mask_decoder.py:301-305), mixing examples and "
                                  "classes")
    if rate != 8 and segment_example_logits:
        raise NotImplementedError(f"classification_layer_downsample_rate={rate} together with segment_example_logits / "
                                  f"embeddings_per_example is not built: la_classify_max takes prototype widths up to 64, and no "
                                  f"reference recipe combines them")
    if levels == 2 and (conv_classification or rate != 8):
        raise NotImplementedError("classification_levels=2 together with conv_classification or classification_layer_downsample_rate != 8 "
                                  "is not built: no reference recipe combines them")


def check_prompt_encoder(prompt_encoder, segment_example_logits, embedding_extraction, levels, conv_classification) -> None:
    """The one check of ``prompt_encoder`` (config_from_kwargs and Lam), on the RESOLVED segment_example_logits."""
    if prompt_encoder is None:
        return
    if prompt_encoder != "TokenPool":
        raise ValueError(f"prompt_encoder={prompt_encoder!r}: None (the plain prompt encoder) or 'TokenPool' (build_lam.py:121,181)")
    if embedding_extraction is not None:
        raise NotImplementedError("prompt_encoder='TokenPool' together with embedding_extraction is not built: the token means replace "
                                  "the stream's embeddings, and no reference recipe combines them")
    if segment_example_logits:
        raise NotImplementedError("prompt_encoder='TokenPool' together with segment_example_logits / embeddings_per_example is not built: "
                                  "no reference recipe combines them")
    if levels == 2:
        raise NotImplementedError("prompt_encoder='TokenPool' together with classification_levels=2 is not built: no reference recipe "
                                  "combines them")
    if conv_classification:
        raise NotImplementedError("prompt_encoder='TokenPool' together with conv_classification is not built: no reference recipe "
                                  "combines them")


def check_fusion_transformer(fusion_transformer, has_image_encoder, segment_example_logits, embedding_extraction, levels,
                             conv_classification, rate, prompt_encoder) -> None:
    """The one check of ``fusion_transformer`` (config_from_kwargs and Lam), on the RESOLVED segment_example_logits."""
    if fusion_transformer == "TwoWayTransformer":
        return
    if fusion_transformer != "OneWayTransformer":
        # IdentityTransformer included: the reference's MaskDecoderLam.forward calls its transformer with four arguments and
        # IdentityTransformer.forward takes three (transformer.py:21), so the reference itself cannot run it
        raise NotImplementedError(f"fusion_transformer={fusion_transformer!r} is an off-path ablation of the reference; only "
                                  f"'TwoWayTransformer' and 'OneWayTransformer' are built")
    if has_image_encoder:
        raise NotImplementedError("fusion_transformer='OneWayTransformer' is built for models without an image encoder (use_vit=False, "
                                  "the reference's lam_no_vit, which every reference recipe with this switch builds); with an image "
                                  "encoder in the model it is an off-path ablation still")
    pairs = (("segment_example_logits / embeddings_per_example", segment_example_logits),
             ("embedding_extraction", embedding_extraction is not None),
             ("classification_levels=2", levels == 2),
             ("conv_classification", conv_classification),
             (f"classification_layer_downsample_rate={rate}", rate != 8),
             (f"prompt_encoder={prompt_encoder!r}", prompt_encoder is not None))
    for name, on in pairs:
        if on:
            raise NotImplementedError(f"fusion_transformer='OneWayTransformer' together with {name} is not built: no reference recipe "
                                      f"combines them")


def config_from_kwargs(**kw) -> LamConfig:
    """Build a LamConfig from reference-style kwargs, rejecting off-path ablation switches."""
    kw = dict(kw)
    for k, dflt in _OFF_PATH_DEFAULTS.items():
        if k in kw:
            v = kw.pop(k)
            if k == "dropout":          # an inference no-op (eval mode), accepted like the reference does; LamTrainer raises on != 0
                kw["dropout"] = float(v or 0.0)
                continue
            if v != dflt:
                raise NotImplementedError(f"{k}={v!r} is an off-path ablation of the reference; only {dflt!r} is built")
    fields = LamConfig.__dataclass_fields__
    unknown = [k for k in kw if k not in fields]
    if unknown:
        raise TypeError(f"unexpected LabelAnything arguments: {unknown}")
    kw["segment_example_logits"], kw["embeddings_per_example"] = resolve_examples(kw.get("segment_example_logits", False),
                                                                                  kw.get("embeddings_per_example"))
    check_prompt_encoder(kw.get("prompt_encoder"), kw["segment_example_logits"], kw.get("embedding_extraction"),
                         kw.get("classification_levels", 1), bool(kw.get("conv_classification", False)))
    check_fusion_transformer(kw.get("fusion_transformer", "TwoWayTransformer"),
                             bool(kw.get("use_vit", True)) and kw.get("encoder", "vit_b") is not None, kw["segment_example_logits"],
                             kw.get("embedding_extraction"), kw.get("classification_levels", 1), bool(kw.get("conv_classification", False)),
                             kw.get("classification_layer_downsample_rate", 8), kw.get("prompt_encoder"))
    check_extraction(kw.get("embedding_extraction"), kw["embeddings_per_example"], kw.get("embed_dim", 256))
    check_levels(kw.get("classification_levels", 1), kw["segment_example_logits"])
    kw["conv_classification"] = bool(kw.get("conv_classification", False))
    check_classification(kw.get("classification_layer_downsample_rate", 8), kw["conv_classification"], kw["segment_example_logits"],
                         kw.get("classification_levels", 1))
    cfg = LamConfig(**kw)
    if cfg.pool_side > cfg.grid:
        raise ValueError(f"embeddings_per_example={cfg.embeddings_per_example} pools {cfg.pool_side} x {cfg.pool_side} bins from a "
                         f"{cfg.grid} x {cfg.grid} grid")
    if cfg.class_encoder is not None and cfg.class_encoder.get("name") != "RandomMatrixEncoder":
        raise NotImplementedError("only RandomMatrixEncoder is built as class_encoder")
    return cfg
