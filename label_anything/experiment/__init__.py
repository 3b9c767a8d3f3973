"""Mirror of the reference's ``label_anything.experiment`` package for the part the hot path builds: query substitution."""
