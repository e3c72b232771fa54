"""PlanarQuadruped model parameters (mirror of src/planar_quadruped.jl:11-26)."""
from __future__ import annotations

from dataclasses import dataclass


@dataclass(frozen=True)
class PlanarQuadruped:
    g: float = -9.81   # gravity
    mb: float = 10.0   # body mass
    mf: float = 0.1    # foot mass
    lb: float = 0.5    # body length
    l1: float = 0.25   # thigh length
    l2: float = 0.25   # calf length

    @property
    def Ib(self) -> float:
        return self.mb * self.lb**2 / 12  # src/planar_quadruped.jl:41

    def plant_parameters(self):
        """(g, mb, mf, lb): what the dynamics read, in the order of a per-problem plant model (QLN_MODEL_NP)."""
        return (self.g, self.mb, self.mf, self.lb)


def plant_models(models, B: int):
    """A PlanarQuadruped (tiled) or a sequence of B of them -> the (B, 4) float64 numpy array of (g, mb, mf, lb) rows that
    HybridNLP.tracking_rollout_model takes as `model` (move it to the device with torch.from_numpy(...).cuda())."""
    import numpy as np

    if isinstance(models, PlanarQuadruped):
        models = [models] * B
    if len(models) != B:
        raise ValueError(f"{len(models)} models for a batch of {B}")
    return np.array([m.plant_parameters() for m in models], dtype=np.float64).reshape(B, 4)


def state_dim(_model=None) -> int:
    return 15  # src/planar_quadruped.jl:25


def control_dim(_model=None) -> int:
    return 5  # src/planar_quadruped.jl:26
