"""Function representations used as closures: the Legendre family, light spots, ``TrainableScalar`` (a scalar of the
equation, such as kappa, as a trainable entry); ``cnn.PeriodicCNN`` (a torch module, imported on
demand: ``from pde_opt_amd.numerics.functions.cnn import PeriodicCNN``) and ``mixer.Mixer2d`` (likewise:
``from pde_opt_amd.numerics.functions.mixer import Mixer2d``) as ``mu`` of CahnHilliard2DPeriodic."""

from .lights import GaussianSpot, GaussianSpots
from .legendre import (
    ChemicalPotentialLegendrePolynomials,
    DiffusionLegendrePolynomials,
    LegendrePolynomialExpansion,
)
from .scalar import TrainableScalar

__all__ = [
    "GaussianSpot",
    "GaussianSpots",
    "LegendrePolynomialExpansion",
    "DiffusionLegendrePolynomials",
    "ChemicalPotentialLegendrePolynomials",
    "TrainableScalar",
]
