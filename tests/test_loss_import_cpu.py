"""CPU: the reference's import line ``from label_anything.loss import LabelAnythingLoss`` resolves to the device implementation."""
import labelanything_amd.loss as device_loss


def test_reference_import_line_resolves_to_the_device_loss():
    from label_anything.loss import LabelAnythingLoss, PromptContrastiveLoss
    assert LabelAnythingLoss is device_loss.LabelAnythingLoss
    assert PromptContrastiveLoss is device_loss.PromptContrastiveLoss
    crit = LabelAnythingLoss({"focal": {"weight": 0.9}, "prompt_contrastive": {"weight": 0.1}}, class_weighting=True)
    assert list(crit.state_dict()) == ["prompt_components.prompt_contrastive.t_prime", "prompt_components.prompt_contrastive.bias"]
