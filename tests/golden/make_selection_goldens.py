#!/usr/bin/env python3
"""Golden fixtures for the smoothness metrics behind ``bayesian_prior_selection``, produced by the REFERENCE's own
``utils.py`` (/root/reference/utils.py, imported — never copied — behind the import stubs of make_goldens.py).  Two stand-ins
replace what the image lacks: a working ``torchvision.transforms.Normalize`` (per-channel ``(x - mean) / std``, what
torchvision's does to a float NCHW tensor) and ``TinyLPIPS`` below for the LPIPS network, whose weights are third-party and
not available offline.  Everything the fixture pins — the Gini index, the normalisation arithmetic on whatever range the images
come in, the order of the pairs, the triple (1 - gini, mean, max) — is the reference's arithmetic.

The inputs regenerate from the seeds below (``gini_vectors`` / ``image_stacks``; tests import them from here); the file holds
OUTPUTS only.

Output: selection_goldens.npz          usage:  python tests/golden/make_selection_goldens.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


class TinyLPIPS(torch.nn.Module):
    """Seeded stand-in for ``lpips.LPIPS``: two small convolutions, channel-normalised features, the spatial mean of the squared
    feature difference of each — the shape of the LPIPS computation, ``[1, 1, 1, 1]`` per pair like the real one."""

    def __init__(self, seed: int = 7):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.w1 = torch.nn.Parameter(torch.randn(8, 3, 3, 3, generator=g) * 0.3, requires_grad=False)
        self.w2 = torch.nn.Parameter(torch.randn(12, 8, 3, 3, generator=g) * 0.2, requires_grad=False)

    def features(self, x):
        f1 = torch.relu(torch.nn.functional.conv2d(x, self.w1, padding=1))
        f2 = torch.relu(torch.nn.functional.conv2d(f1, self.w2, stride=2, padding=1))
        return [f / (f.pow(2).sum(1, keepdim=True).sqrt() + 1e-10) for f in (f1, f2)]

    def forward(self, a, b):
        return sum((fa - fb).pow(2).sum(1, keepdim=True).mean((2, 3), keepdim=True)
                   for fa, fb in zip(self.features(a), self.features(b)))


class Normalize:
    """``torchvision.transforms.Normalize`` on a float tensor [..., C, H, W]."""

    def __init__(self, mean, std):
        self.mean, self.std = mean, std

    def __call__(self, x):
        mean = torch.as_tensor(self.mean, dtype=x.dtype, device=x.device).view(-1, 1, 1)
        std = torch.as_tensor(self.std, dtype=x.dtype, device=x.device).view(-1, 1, 1)
        return (x - mean) / std


def gini_vectors():
    """name -> distance vector: lengths 0 and 1, equal entries, a zero entry, sorted and unsorted."""
    rng = np.random.RandomState(5)
    return {
        "empty": np.array([]), "one": np.array([0.3]), "two_equal": np.array([0.25, 0.25]), "two": np.array([0.1, 0.4]),
        "equal5": np.full(5, 0.125), "with_zero": np.array([0.0, 0.2, 0.5]), "sorted": np.array([0.05, 0.1, 0.2, 0.4, 0.8]),
        "reversed": np.array([0.8, 0.4, 0.2, 0.1, 0.05]), "unsorted": np.array([0.31, 0.07, 0.52, 0.11, 0.29, 0.4]),
        "random6": rng.uniform(0.01, 1.0, 6), "random11": rng.uniform(0.01, 1.0, 11),
        "float32": rng.uniform(0.01, 1.0, 7).astype(np.float32), "spike": np.array([1e-3, 1e-3, 1e-3, 0.9]),
    }


def image_stacks():
    """name -> (5, 8, 8, 3) image stack: uint8 0 .. 255 (what the pipelines return) and float 0 .. 1."""
    rng = np.random.RandomState(6)
    ramp = np.linspace(0.0, 1.0, 5)[:, None, None, None]
    base, other = rng.uniform(size=(1, 8, 8, 3)), rng.uniform(size=(1, 8, 8, 3))
    path = (1 - ramp ** 2) * base + ramp ** 2 * other + 0.02 * rng.standard_normal((5, 8, 8, 3))     # uneven steps along a path
    return {
        "uint8": rng.randint(0, 256, size=(5, 8, 8, 3)).astype(np.uint8),
        "uint8_path": (np.clip(path, 0, 1) * 255).astype(np.uint8),
        "float": rng.uniform(size=(5, 8, 8, 3)),
        "float_path": np.clip(path, 0, 1).astype(np.float32),
    }


def import_reference_utils():
    stubs = {"bayes_opt": ["BayesianOptimization", "SequentialDomainReductionTransformer"],
             "lpips": ["LPIPS"], "torchvision": [], "torchvision.transforms": ["Normalize"]}
    for name, attrs in stubs.items():
        m = types.ModuleType(name)
        for a in attrs:
            setattr(m, a, type(a, (), {}))
        sys.modules[name] = m
    sys.modules["torchvision.transforms"].Normalize = Normalize
    sys.path.insert(0, "/root/reference")
    import utils
    return utils


def main():
    utils = import_reference_utils()
    model = TinyLPIPS()
    out = {}
    for name, d in gini_vectors().items():
        out[f"gini_{name}"] = np.array(utils.compute_gini(d), dtype=np.float64)
    for name, images in image_stacks().items():
        out[f"lpips_{name}"] = np.asarray(utils.compute_lpips(images, model), dtype=np.float64)
        out[f"triple_{name}"] = np.array(utils.compute_smoothness_and_consistency(images, model), dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, "selection_goldens.npz"), **out)
    for k, v in out.items():
        print(k, v)


if __name__ == "__main__":
    main()
