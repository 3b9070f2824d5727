"""Geometry of the limb forward model with gradients (nemesisLfmg, ForwardModel_0.py:1372-1521) in the form the fused engine call
`AnsfmEngine.cirsradg_ck_limb` takes it: the interpolation of the limb paths to the tangent heights of the measurement
(:1475-1496) as a mixing matrix C (NGEOM, NPATH), MOD = SPECOUT @ C.T.

BASEH_TANHE of :1444-1446 is :1180-1182 of nemesisSOfmg and the loop of :1475-1496 is :1211-1232, line for line (the nearest
path by argmin, `base0 <= TANHE` choosing the neighbour, a lower neighbour of -1 wrapping to the last path, weight 1 on the lower
path above the top one, the weights 1 - fhl and 1 - fhh); only the arrays they mix differ.  So the occultation's two functions
are this model's."""
from .occultation import tangent_heights_km, tangent_mix  # noqa: F401
