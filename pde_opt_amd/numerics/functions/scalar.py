"""A scalar of the equation as a trainable entry of ``opt_parameters``.

The reference's parameters are a pytree: a float such as ``kappa`` is a leaf like any other and JAX differentiates
through it.  Here a trainable scalar is named explicitly, ``opt_parameters={"kappa": TrainableScalar(0.002)}``: a plain
float stays fixed data and is refused among ``opt_parameters``.  ``PDEModel.train`` / ``optimize`` return a
``TrainableScalar`` under the same key and ``PDEModel.solve`` unwraps it.
"""

from __future__ import annotations

import math


class TrainableScalar:
    """``value`` with the variable the optimiser moves.

    ``positive=True`` (the default, and the right choice for kappa): the variable is ``q = log(value)``, the Jacobian
    column is ``d/dvalue`` times ``value``, and no step can produce ``value <= 0``.  ``positive=False``: the variable is
    the value itself; a trial the equation cannot take (``kappa <= 0``) is a rejected step of Levenberg-Marquardt and a
    failed line-search point of BFGS, never a solve."""

    def __init__(self, value, positive: bool = True):
        self.value = float(value)
        self.positive = bool(positive)
        if not math.isfinite(self.value):
            raise ValueError(f"TrainableScalar({value!r}): not a finite number")
        if self.positive and not self.value > 0.0:
            raise ValueError(f"TrainableScalar({value!r}, positive=True): the value must be > 0 (its logarithm is the "
                             "optimiser's variable); pass positive=False for a scalar that may change sign")

    def __float__(self) -> float:
        return self.value

    def variable(self) -> float:
        """the optimiser's variable: ``log(value)`` or the value"""
        return math.log(self.value) if self.positive else self.value

    def with_variable(self, q: float) -> "TrainableScalar":
        """the scalar at variable ``q`` (same ``positive``)"""
        out = TrainableScalar.__new__(TrainableScalar)
        out.value = math.exp(float(q)) if self.positive else float(q)
        out.positive = self.positive
        return out

    def column_factor(self) -> float:
        """``d value / d variable``: what scales the tangent ``du/dvalue`` into the optimiser's column"""
        return self.value if self.positive else 1.0

    def __repr__(self) -> str:
        return f"TrainableScalar({self.value!r}, positive={self.positive})"
