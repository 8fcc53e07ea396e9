"""The reference's RandomFourier (xenoverse/utils/random_nn.py:346-368) over numpy's stream, in its draw order: the LinDS
command, the AnyMDP potential and the AnyHVAC sensor drifts and heat curves are all built from it."""
import numpy as np


class RandomFourier(object):
    """y(t) = sum_k c_k[:,0] sin(w_k t/max_steps) + c_k[:,1] cos(w_k t/max_steps); w_0 = 0, 1..max_item further terms"""

    def __init__(self, ndim, max_order=16, max_item=5, max_steps=1000, box_size=2, rng=None):
        rng = rng if rng is not None else np.random
        n_items = rng.randint(1, max_item + 1)
        self.coeffs = [(0, rng.normal(size=(ndim, 2)) * rng.exponential(scale=box_size / np.sqrt(n_items), size=(ndim, 2)))]
        self.max_steps = max_steps
        for _ in range(n_items):
            order = rng.randint(1, max_order + 1) + rng.normal(scale=1.0)
            factor = rng.normal(size=(ndim, 2)) * rng.exponential(scale=box_size / np.sqrt(n_items), size=(ndim, 2))
            self.coeffs.append((order, factor))

    def __call__(self, t):
        x = t / self.max_steps
        y = 0
        for order, coeff in self.coeffs:
            y = y + coeff[:, 0] * np.sin(order * x) + coeff[:, 1] * np.cos(order * x)
        return y
