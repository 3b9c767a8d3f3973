"""The image encoder's launch sequence, pinned on the CPU (tools/encoder_trace.py): every public function of ``_lib`` is a recorder,
``LamEngine.encode_images`` runs on two zero images, and the trace - function, arguments, tensor shapes / dtypes / strides / storage
aliases, in launch order - is compared by length and sha256 with the one recorded when the table below was written.  A change to the
host driver that is meant to launch the same work leaves every row as it is; one that is meant to change a launch re-records its rows
(``python tools/encoder_trace.py --table``) and says so.

What the rows reach.  SAM, 768 wide, 12 heads, depth 3 (two 14 x 14 window blocks, one global): at 1024 px the 64 x 64 grid - folded
LayerNorm on the plane-pair stream (default), the LayerNorm kernels (nofold), the V^T / window-scatter attention (norows), second weight
planes instead of token means (planes), no split precision, bf16, no SAM neck, want_last_block; at 448 px a 28 x 28 grid (global block on
la_relpos_terms, padded windows); at 256 px 16 x 16 (in-kernel rel-pos, windows wider than the image); 20 x 20 windows at 640 px (the
only windows beyond 16 slots); the reduced fixtures' sam_tiny; 80-wide heads padded to 128.  HF, 768 wide, depth 2: folded and
LayerNorm-kernel stacks at 224 px, V^T attention, fp8 QK^T, 96 px (37 tokens: below the fold's group size), hf_tiny with a resampled
position table, 32-wide heads padded to 64.  DINOv3 (five prefix rows from the weights, no position table, la_rope_qk on q and k,
LayerScale folded into the packed weights), 768 wide, depth 2 at 192 px (149 tokens): the folded stack, the LayerNorm kernels, V^T
attention; the reduced fixtures' dinov3_tiny and dinov3_hd32 (32-wide heads: the first 32 of every 64 columns rotated) at 64 px.  DINOv2
(patch 14, LayerScale folded likewise), 768 wide, depth 2: at 168 px (145 tokens) the folded stack and the LayerNorm kernels on a
resampled table, at 224 px the table as stored; dinov2_tiny at 70 px, and at 42 px (resampled table, la_im2col_patch_pad); dinov2_hd32.

The TRAINING graphs (train_encoder.py) have a table of their own, EXPECTED_TRAIN: forward, then backward of an all-ones gradient, on two
zero images, with the gradient slots laid out in one flat buffer as FlatAdamW does.  Each row is pinned twice: the full trace, and the
shape trace with the storage numbers masked.  The table was recorded with the four hand-written block copies that the one block stack of
train_encoder.py replaced (forward and _backward_scaled of HfEncoderGraph and of SamEncoderGraph); the shape digests and the full digests
of the HF rows are from that recording, unchanged.  The full digests of the SAM rows were re-recorded with the one stack, which aliases
what the SAM copy allocated afresh: V^T and the attention backward's dO, dq | dk | dv, D, d relh, d relw, window-order dY and dX are one
set per block geometry (windows, global) instead of one per block, and a global block's dX of q | k | v goes where fc1's dX went, as in
the HF copy.

What the rows reach.  hf_tiny at 240 px: resampled position table, widths that are no multiple of 256 (exact-fp32 weight gradients),
unfused GELU; at 224 px the table as stored.  HF 768 wide at 224 px: la_gemm_tn16, the fused q | k | v weight gradient, and the GELU
epilogues with la_gemm_fused_act_ok answering yes and no; then exact-fp32 weight gradients (fast_wgrad off), transposed copies + split-K
(tn16 off), GELU passes (fused_gelu off), the gradient slots laid out and handed over back to front (negative stride between query,
key and value: three la_gemm_tn16 products per block on purpose, none with gsize), 32-wide heads padded to 64, bf16.  SAM: sam_tiny (one padded-window block, one global block), the same with rel-pos tables of another
length (longer for block 0, shorter for block 1), 768 wide at 448 px (two window blocks of one geometry + one global) with the GELU
epilogues on and off, 80-wide heads padded to 128.

The DECODER half of LamEngine has the third table, EXPECTED_DECODER, in the same form: ``prompt_encoder``, ``mask_decoder`` and
``postprocess_dev`` (with ``example_valid`` where segment_example_logits is set) on zero tensors, called with the arguments ``Lam._run``
passes; the last line records every tensor of the prompt encoder's result and of the output, so which results are arena views and which
clones is pinned too.  ``Tensor.pin_memory`` is an identity while a row runs, ``selected_rows`` is always passed, and the host predicates
that ask the shared library answer what the row states: la_stream_mlp_ok yes, la_extract_pool_plan (64, 2, 4096), la_conv3x3_split_ok yes
except in the last row.  The table was recorded from the decoder drivers as they stood BEFORE their repeated launch groups became shared
steps (one hand-written copy per method), with this tool unchanged; the shared steps reproduce it.

What the rows reach.  One episode, 2 supports, 3 classes, a 4 x 4 grid (16 stream rows a slab), 2 points + 1 box + a 16 x 16 mask per
(support, class) pair; the encoder (sam_tiny) is built and never run.  64 wide - the unfused chain on an fp32 decoder, im2col spatial
convolutions: all three prompt kinds, points only (adds the padding token), boxes only, masks only (the single "no sparse" token), the
three merge attentions with a class-encoder bank.  256 wide, all prompts: the fused two-way kernels + la_conv3x3_split (default), "f16x2"
(plane-pair image-side operands: in the upscaler behind the fused kernels, and throughout the chain with fuse_twoway off),
decoder_dtype=None (16-bit operands, im2col convolutions), fuse_twoway off, conv_split off
(la_conv3x3_f32), 33 classes (the mask decoder above fused_ok's 32 tokens, the prompt encoder still fused), no spatial convolutions.
OneWayTransformer: fused with the chain MLP (the default threshold at this size), fused with la_stream_mlp (ONEWAY_MLP_MIN_ROWS = 0),
fuse_oneway off, "f16x2" (the chain through the fp32 hidden layer) with fuse_oneway on and off.  TokenPool: with masks, without, masks
only (ns = 1: no token mean), 9 classes x 4 tokens = 36 with a bank (the unfused chain on pooled slabs).  Heads and extraction:
cross_attention with 2 queries and segment_example_logits (fp32, and 16-bit operands: the extra cast of the pooled output),
embeddings_per_example = 4 (2 x 2 region means, la_classify_max), two levels, conv classification, downsample rate 1 (256-channel map:
la_conv3x3_split_ok answers no, la_classify_wide)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import encoder_trace as T          # noqa: E402

EXPECTED = {
    'sam 1024 default': (37, '2dd4a5c2cf1aef435ff5982d2a2361be62a81e583a6ba86db8782e52034851da'),
    'sam 1024 nofold': (38, 'e3d33be2c997107b11d3e7e4e37882aea80bdf604d8a4586ad67a0dfe8dcd91e'),
    'sam 1024 nofold norows nocs': (38, 'ae35ef5c34a5908e8b8675bf7e18daef72fd8a70941c609852952fd7fb811cfa'),
    'sam 1024 planes': (32, '6537ce7ec6a4888077e8503fd8a5ebb725a193b931e9f2645b228ebdfbeaa6e3'),
    'sam 1024 planes norows': (32, '55b1fa739a2d4995add90244f1d87be9b11c1f3daa4476ec87fff5ce3aa84ad8'),
    'sam 1024 imprecise': (29, 'e5def9bf82cc4e0b0e15ae7ec1cc8a73fb87398f45a4e8744550ebc3a76682ca'),
    'sam 1024 bf16': (28, '894e3bb69c866b6ecb0bc91850a812c082ba3476555186e3c7dda19b148262e6'),
    'sam 1024 no neck': (33, 'b5f34772bf15a4f0f96844ca6547308822fa107a7fef4373f2f38fca4cfaaf21'),
    'sam 1024 last block': (37, '956451f117973dd1f25e6334848462f0bfdaabf245111dedf8411e3c1bdf8e1d'),
    'sam 1024 last block nofold': (38, '2988d3e4537910d4ce944354d555e7f0f7d7d2f3fdf2298c32a8837f0a8ba69c'),
    'sam 448 default': (39, '639319a536fc84f2bdeb6f54cd989a270c98257ba16a9de38a4f191aea3a9014'),
    'sam 448 norows': (39, '73408290b43c0f46fb24c87abc628eb21e7f63c184f85d94618c73bc7d8671e7'),
    'sam 256 default': (39, 'cfde682b7ce4be1b1d84106e1f70782d3898bd4c3bb81123c26c9b9c5a1d1bb4'),
    'sam 640 window 20': (41, '970d85b4c4419539115a1d58285d56cb1f315ea0e21173bb09bebef97b32e165'),
    'sam_tiny': (23, '0a68e30050c975a174c84d22ede4463ad7b5d8669bf7538f694fcf0ddcf4a76b'),
    'sam_tiny norows': (23, '5eb908b8bcb4f4640b021c7c5d1f657ff31cbe63cd7f958c1c52cddccfa48392'),
    'sam hd80 448': (23, 'e4d803ec8b38cd8b5805dcbf4d1b34d5f664884c2d42329619166b41533cf1e0'),
    'hf 224 default': (26, '58e4ea5247d6b3218402821a407c5793ae8b77c27629a09634d7affcdbd7a9f6'),
    'hf 224 nofold': (24, '88992175630469b8dc756f6a73ed7d75e7b3867ac2457dfa02aec87e96314cd5'),
    'hf 224 nofold norows': (24, '9318bd9cc63fa76070d3d19cc82d111496ee7b021f711856d8d59c1c1e4300bd'),
    'hf 224 fp8': (26, '5f4055216f864456a4841524f50ae11823e0e73d5085fc6516cb3bbd21f38513'),
    'hf 96 default': (25, '1d7d6f67575faf9947ee7181dcd185ae10c7a213318e089f8effe097c18b8ced'),
    'hf_tiny 240': (19, '90ac544736b1a2f491e33b0e29743b74c96d20e2773dd593e20d17fd5cd4f86a'),
    'hf hd32 160': (19, '0fc307c677c6ebd002ffed0a3518237d7dbfd690bae86ced86831027c31d717c'),
    'dinov3 fold 192': (28, 'fc84d67db4cfd4e2837eb49ddb7eec9896628f77ddd6ea4200f7777c4ffd3ca9'),
    'dinov3 fold 192 nofold': (26, '379a3b1c5463bceaa23a1b80857e55c78812a548540d86c0f08e6934f2df2de9'),
    'dinov3 fold 192 nofold norows': (26, 'f8a95d20ae38456ac920f1c6e153452800ad6d675179a1be06a0d88069a870dd'),
    'dinov3 tiny 64': (20, '38f53994fc563cee6bb5eb503a593e3704dbee700b12e0f0723d9997f8065ac7'),
    'dinov3 hd32 64': (20, '3efba6e7bf4da9873f0df2c43440a8f37711cd6ab7b1b42a08c10fc8ef0738d4'),
    'dinov2 fold 168': (27, 'd4a04decee65af08459534ec742a62ee4767d7cdc360d672add7db61812d9690'),
    'dinov2 fold 168 nofold': (25, 'ea5676bb089e32ff404212d316d30aafd97e4acbbff6cbe1753c3a2da25b4ba7'),
    'dinov2 fold 224': (26, 'abfc0b9a3ea23488dd80e701815e9b9969ab36a48d1c2379d5e6a027f8a5f526'),
    'dinov2 tiny 70': (18, 'e3f31178de6259593162860c3f2ef1c471ba457155783c9f7c2eaeb496d185ed'),
    'dinov2 tiny 42': (19, '0537fd8ccefb197b8f59dafb032ba05650514386d2f937210c0bcb8a83ac9d71'),
    'dinov2 hd32 70': (18, 'f464a969d09050e7a1cefff8271ea968c6e3062d7eea8a2bd4361e07aa008bba'),
}

# name: (number of lines, sha256 of the full trace, sha256 of the shape trace) - python tools/encoder_trace.py --train-table
EXPECTED_TRAIN = {
    'train hf_tiny 240': (104, 'f00bf8744e831e965485a6433101432edc5aa199ebf52806d7d9995f99445787',
                              '56925bb9c4d90f9db792e5cbf00dda00d6ca14ab1da68c9fd66ff27067172f70'),
    'train hf_tiny 224': (102, '55a559359d346be20330a65e7fa3624c612b0dc9421c08d32eca1451543851f3',
                              '5f70876bfd853b7ccf47fadb1dfa17c3cae7cac1f3dd8e8961f6062fcc0bb112'),
    'train hf 224 fused act': (62, 'db52b4b3da498636eb047f15e900cc5192b7dd5770ec131d2fd10239b99883e2',
                                   '36e89dd2e3ba63d05a94798b4976e451dbaec1d6ec1ef40ccaddd80548224e75'),
    'train hf 224 unfused act': (66, '07812948169e2f139577c942d10c1411ca93f053f114f7fdadeb2c28fdb2e08d',
                                     'b1fdd319ac0087506356b8570495358e6963edf3dbc77b319926d5a43a7dfc97'),
    'train hf 224 exact wgrad': (98, 'bf9eb3a127f86222056bffd117fd1b2f7cd79e5e08091c8e15bff0b05b58e4b2',
                                     'd06ab4be073ce180c92a7148854e49f682c4f3340271694c3d65243d636c4f16'),
    'train hf 224 no tn16': (78, 'df58d7ae6d38848928aa45bc47dd09b5c58df79edfdf30f413d3acb995a468d3',
                                 'd33d77d5b22373f49b1c2e4063760a4e4c1655d4e0c10446fb975912bca15dcb'),
    'train hf 224 no fused gelu': (62, '0b5e0c3d35071acae614dae9fb55bb357d4c5d39c0d1eb21624b30e6d215fc7f',
                                       'e7c0ad9e52cc7e340c5338c155d6423d2385a520cbb8a4ef5db2caf3a95c2190'),
    'train hf 224 reversed slots': (66, 'c2a9e2993663088318084935f68afbdeaf76e5d57c83d20b3f24a8e3dfb6fad6',
                                        '5ccead187f6499b34492ea8fd981b79518e395b866abb360edf0932258ac3ed3'),
    'train hf hd32 160': (104, '6f3845d2c07e70d12ed18d154181acdea65a790e265334cfffbddc1efe5a45ac',
                              '6fa9fa943861fb64ac315c422baa0699f490e9b8c177aaf8eca05fc2be8c4cbc'),
    'train hf 224 bf16': (62, 'e4764caf4b279f1f421a3d8ae4ccbfb75a3cdf28443006739cbcbd73ebebf0b9',
                              'd74be701ced495b27c9c587fdd4667cfb5b6cbd25694440f3c612d988b3ae60d'),
    'train sam_tiny': (92, '6d7efaf2bff2d973e6195562d0c80517de06632ff5ff78cb0d7bd9608358ebd9',
                           'db723e8463cca01412773bfb37a8be3fbe6dbef99993b6f7e12a30f56791d3d4'),
    'train sam_tiny resampled rel-pos': (100, '8c44b4c25fb5c2c8e9bb448cee5da959181f9042bc22549b0516685285b35821',
                                             '5ad3437b1af68f77c35bb6014b7cb3ff3b007440e843b5893c440b05385bfdea'),
    'train sam 448 fused act': (94, '7796d8ed3c7ee70a5f95612d773de60862503085329ee189026eaa793ac834ee',
                                    'b45df100cb321352bc71ae0b2dd0c43c9dfef603e51961dbd5b81fb3eb1aa0e6'),
    'train sam 448 unfused act': (100, '2ede3a32bc399b789746cbe9dd415dce90e94585ab4b379cc6e1711cb66b181c',
                                      '94d48e7b85117ec692370506434fa0d2303028fc5aea9bf97e1cb85f4031d09c'),
    'train sam hd80 448': (90, '09315ed0d8cf3925d65957fb811f846fecd1b8ef7469cedb2fde106000c272e2',
                               '18b3eb1b5aa65ea525d915cf0406ba7afd5e641732c9076079b0355d1297e91a'),
}

# name: (number of lines, sha256 of the full trace, sha256 of the shape trace) - python tools/encoder_trace.py --decoder-table
EXPECTED_DECODER = {
    'dec 64 all prompts': (127, 'ae4e528f5dab571f4801a1773a1358d0716526d03ec703ff42a4a07f4de88b42',
                               '2d8446eda767b2b48e39165311e04def36eaa283d55fb96966c36de66140ff11'),
    'dec 64 points': (127, '89fe4d5aedc7a9fda1229281894298ce0c7a155202c6730213272adf53bf555f',
                          '414cb9ba5fc728e9262ac82f97353c5442151de338799fce51b1bed5478496f0'),
    'dec 64 boxes': (127, '62228987496626888e911a2a0dcb4e72287fbe0dbd0c3c916b5d7681c0494064',
                         '20c719bace5faf4fde350b9e908c0c032ef46aeb23d2ab03654ccb08e41af173'),
    'dec 64 masks': (127, '61adbcc496adf451d706fe27a7acb838acfcf2c134cf824aaa989347752549b2',
                         '3ca3c362443bb59d0192da42aed4e0501c5a8e2356c563e7af46a950538d787e'),
    'dec 64 merge attentions bank': (144, '8109518c8bd1d64469541ab4365413e23fe35165e28215658ce67bb9150748fa',
                                         '6041c5489cfae342107690940d356b8527f977af474f6ab21d63fc76f5c870c9'),
    'dec 256 fused': (122, 'ee90592bb085432a241210a97fc9cd6f588058dba8643128cfbbaf1c33386eae',
                          '2266f7552c3660949a58ff4bf6612ff7a0fcbb1fd4a873dd33eb9fb40e6e20f6'),
    'dec 256 f16x2': (123, '9bf49e687145700f99f5e151c18705f1be0ebe8dfa17d341653db7f9d89e4ba7',
                          '665a295f05d664c4f39ee73585bc35e8d6222f936bd901493e8705b13838a2a6'),
    'dec 256 f16x2 unfused': (128, '7b96dc6d18a5cae5b8f4e6e0e6e19fa208dbb418bb97812399c66513c8022a02',
                                  '455d8c9c731f01cbce06bea3b67a25238bbb64976f2d409e8698c07081630317'),
    'dec 256 16-bit im2col': (127, '6eead523d8d61a20a9abdc2504f8f0bda63565f41b742e6245ee441c4bf9ecfd',
                                  'a1955dc189fe53b9ce52e04f35ebf1d83818a9214d857883468bf28777455168'),
    'dec 256 unfused': (127, 'bc6ba4e4bd9885c5a385a5048fec0fa893cd0c27ce16e2409e40b8e59a26c02b',
                            '4db6758efedd6cc87750ce9f1d9a65cd9713bc2d51bacdfef404332020dfe89f'),
    'dec 256 conv_split off': (119, '2f9e76c7b324a04d2c6a8e8927447c73c757cabbb6d7e0395fc0cbb2a6b56348',
                                   'ef3481ff7ffa7ceef5a5628eb6d68df03310a6d018d71c2d65c50582cb98f7d7'),
    'dec 256 33 classes': (125, '3c169210fc835e53a96aed9fca84de0e05458753444b0466421fd024b4ab503d',
                               '02a1a00a0e5366984586b5f843a52f4a4cca7cf2c07b890c512eda6abf6226cf'),
    'dec 256 no spatial convs': (114, 'ee764d315941b3f234ee7d8d151ab820f47a3308314dd9e597955c1fc4320156',
                                     'b77497a6ecf93fd07b0e6406f8b9371622522dc5b55a8c3d9cf46d948d8f1cc7'),
    'dec oneway fused chain mlp': (98, '2df5e9c722e1dfb018c8df3ac26764b5b76651dac3f394fe3a8d5bea54c964f0',
                                       '4e110a886515da875d8c5ab61c871af4ea00526acf2b81d300ee4e44ddef26ba'),
    'dec oneway fused stream_mlp': (92, '3fc49dc2e43a3cba56a8cd1e7a85a8758d8664f768e603b5b8bb152f33edf618',
                                        '52a54f90fb2bed7ea61b3a72466359fc7d45b73ef4526b2f90cb44d7c0f7e50f'),
    'dec oneway unfused': (98, '33fc66631317a2eff085d0ec82ccfbe9614310734293bd867d8fcbebe6eaf606',
                               'ef78ea88d810ee3b2863813f4859900cb41381ef1351b636d38fbc0eed4fde02'),
    'dec oneway f16x2': (101, '97b140ff19de732a5bd63ed19b67b530a855079cb0617f034d4dd9cdd34feecd',
                             '164b7d1c8afc2a70ea281bedda89e7b7f79f0972303663d135e45ac60a58dddb'),
    'dec oneway f16x2 unfused': (101, '6a7278c8626d5e94111a9048dbd09c0bbd5870144129b1de91dbb767d8d883a8',
                                     '473e3607132c57f8fa2baf80c7289a60050866b9540f0e04db45f26943f6cc09'),
    'dec pool masks': (128, '1a4175a3d60576c2679391c94e04989391b4689d8d7e8f0e5f4a1e7553be2d99',
                           '3b194c4db13cfa373daf969e1bf62ad8bc9bfb89321a325af8dc4bbb0dd0a6ee'),
    'dec pool no masks': (128, 'caa2fba432e0cc4277d4c238c6974fab41f9ccaad9d34c5374d5aedfe62b3bed',
                              '638d55b7e0c339c71ed07a2cc79adc68e25cc8e74ed6f5c6640b1fac55f0b6d7'),
    'dec pool masks only': (127, '2c38e6be36362ff6e15ce65d37207515d443afd2151b6ab3367d4f1788432b30',
                                'f1c61ea1af3d714358572fcbb45d42582523b7d4e684ee195a3bc7306849d809'),
    'dec pool 36 tokens bank': (131, '1660aba993fe0b30d650cfad490321d726365378bc83f1f7bea541bfc4139ab6',
                                    '0a9676ac32d5a218fe63c9cd9013ccabc0b9360e1b50c82f9a85c4444d068858'),
    'dec cross_attention 2 queries': (131, 'ae1fb7273323c230eeff34abace44f9721a091f547d50006168455e7c176995b',
                                          '815641cb0a45ae8d32fc63e6179dc19933fe2c189113b8b8116548dd622d55d4'),
    'dec cross_attention 16-bit': (138, '68cca3e2d2116691471ff2398a24d6affa5be4871baca0c7c335778af369f0ed',
                                       'a5ac5e432450941fcff6e8fa291ce754c5da596db454f2b05ab9f6961b035ccb'),
    'dec 4 embeddings per example': (122, '5f6ea3f5771512c49f07f5886cb92349af6319305ae3388cb7c3e72265a0a937',
                                         '0fdf9d7bfb11e4f95c359f9a40f39b686204788f53deffb74be7d888e843d3a9'),
    'dec two levels': (124, '99025002481bf3680c3e1803e183f078eaf66b8a13a2c7b667805cd9507941b1',
                           '030f0bf474122d1483f00f57761bc469a3ae75998f835fc85b256338c46b0e52'),
    'dec conv classification': (123, '3986697b0a4c8b687983b0e059a5095767f848a77f00f813a9db074b537bd59b',
                                    '163839c610b38101de9b527bcaea990dff92fba2e3bef0f322cedb6d3b2e832b'),
    'dec downsample rate 1': (122, '039a04eb614e47a38017310cf76292dc164d189befb547153fa57588e6f17fde',
                                  'ffa082d1884931c3800c3f40df13c08d5b9217400bbafd1f024eb2c516f71bb5'),
}


def test_the_table_covers_the_matrix():
    assert list(T.matrix()) == list(EXPECTED)
    assert list(T.train_matrix()) == list(EXPECTED_TRAIN)
    assert list(T.decoder_matrix()) == list(EXPECTED_DECODER)


@pytest.mark.parametrize("name", list(EXPECTED))
def test_encoder_launch_trace_is_unchanged(name, monkeypatch):
    got = T.trace(T.matrix()[name], monkeypatch.setattr).digest()
    if got != EXPECTED[name]:
        print(f"launch trace of {name!r} changed: {got} != {EXPECTED[name]}; inspect it with\n"
              f"  python tools/encoder_trace.py --print {name!r}")
    assert got == EXPECTED[name]


@pytest.mark.parametrize("name", list(EXPECTED_TRAIN))
def test_training_graph_launch_trace_is_unchanged(name, monkeypatch):
    rec = T.train_trace(T.train_matrix()[name], monkeypatch.setattr)
    got = rec.digest() + rec.digest(shape=True)[1:]
    if got != EXPECTED_TRAIN[name]:
        print(f"training launch trace of {name!r} changed: {got} != {EXPECTED_TRAIN[name]}; inspect it with\n"
              f"  python tools/encoder_trace.py --print {name!r}")
    assert got == EXPECTED_TRAIN[name]


@pytest.mark.parametrize("name", list(EXPECTED_DECODER))
def test_decoder_launch_trace_is_unchanged(name, monkeypatch):
    rec = T.decoder_trace(T.decoder_matrix()[name], monkeypatch.setattr)
    got = rec.digest() + rec.digest(shape=True)[1:]
    if got != EXPECTED_DECODER[name]:
        print(f"decoder launch trace of {name!r} changed: {got} != {EXPECTED_DECODER[name]}; inspect it with\n"
              f"  python tools/encoder_trace.py --print {name!r}")
    assert got == EXPECTED_DECODER[name]
