"""The table of encoder kinds (config.ENCODER_KINDS): every kind a registered geometry names has a record, and the one lookup refuses a
kind it does not know by name."""
import pytest

import tests.cases              # noqa: F401  (register the reduced geometries of every family)
import tests.cases_dinov2       # noqa: F401
import tests.cases_dinov3       # noqa: F401
from labelanything_amd import train_encoder
from labelanything_amd.config import ENCODER_KINDS, ENCODER_SPECS, encoder_kind


def test_every_registered_kind_has_a_record():
    kinds = {spec.kind for spec in ENCODER_SPECS.values()}
    assert kinds == set(ENCODER_KINDS)
    for kind in kinds:
        rec = encoder_kind(kind)
        # trainable through a graph class that exists, or refused with a text - never both, never neither
        assert bool(rec.train_graph) != bool(rec.train_refusal)
        if rec.train_graph:
            assert getattr(train_encoder, rec.train_graph).KIND == kind
        assert all(rec.spec_from_hf is not None for _ in rec.model_types)


def test_an_unknown_kind_is_refused_by_name():
    with pytest.raises(ValueError, match="no encoder driver for kind 'swin'"):
        encoder_kind("swin")
