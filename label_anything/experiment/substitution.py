"""Mirror of the reference's label_anything/experiment/substitution.py: the reference's import line
``from label_anything.experiment.substitution import Substitutor`` resolves to the device implementation."""
from labelanything_amd.substitution import Substitutor, generate_points_from_errors  # noqa: F401
