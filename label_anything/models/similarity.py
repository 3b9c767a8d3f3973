"""Mirror of the reference's label_anything/models/similarity.py: the cosine-similarity few-shot segmenter on the device."""
from labelanything_amd.similarity import SimilarityFewShotSegmenter, build_similarity  # noqa: F401
