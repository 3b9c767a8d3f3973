"""Mirror of the reference's label_anything/loss/__init__.py: the reference's import line
``from label_anything.loss import LabelAnythingLoss`` resolves to the device implementation."""
from labelanything_amd.loss import LabelAnythingLoss, PromptContrastiveLoss  # noqa: F401
