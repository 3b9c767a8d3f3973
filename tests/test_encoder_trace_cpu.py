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
position table, 32-wide heads padded to 64."""
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
}


def test_the_table_covers_the_matrix():
    assert list(T.matrix()) == list(EXPECTED)


@pytest.mark.parametrize("name", list(EXPECTED))
def test_encoder_launch_trace_is_unchanged(name, monkeypatch):
    got = T.trace(T.matrix()[name], monkeypatch.setattr).digest()
    if got != EXPECTED[name]:
        print(f"launch trace of {name!r} changed: {got} != {EXPECTED[name]}; inspect it with\n"
              f"  python tools/encoder_trace.py --print {name!r}")
    assert got == EXPECTED[name]
