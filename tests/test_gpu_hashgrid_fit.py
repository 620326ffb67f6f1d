"""GPU: TCNNSDF fits a sphere.  Adam on |sdf - (|p| - 0.5)|^2 plus an eikonal term, p = 2 x - 1 the world point of x in [0, 1]^3;
every step draws a fresh batch from a seeded CPU generator, so the CPU and the GPU run see the same points.

The step count was chosen on the CPU with the plain-torch restatement of the encoding (tests/_hashgrid_oracle.py: restate) in place
of the HIP kernels, same seeds, same head: the loss of the held-out batch falls from 3.92e-1 to 1.02e-2 in 30 steps, 1 / 38 of the
start and so past the 1 / 20 asked of the CPU run (2.92e-3 at 50 steps, 1.81e-3 at 60).  The GPU run must reach 1 / 10 in those 30
steps."""
import json

import pytest
import torch

import _hashgrid_oracle as O

FIT_CFG = (8, 2, 14, 4, 1.5)
STEPS, BATCH, EIK_WEIGHT, LR = 30, 2048, 0.1, 1e-2


def make_field(path, encoding=None):
    """TCNNSDF on FIT_CFG with a 2 x 32 ReLU head; `encoding` replaces the HIP encoding's forward (the CPU restatement)."""
    from iron_amd import tcnn_fields
    L, F, log2T, N, b = FIT_CFG
    conf = {"encoding": {"otype": "HashGrid", "n_levels": L, "n_features_per_level": F, "log2_hashmap_size": log2T, "base_resolution": N,
                         "per_level_scale": b},
            "network": {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 32, "n_hidden_layers": 2}}
    with open(path, "w") as f:
        json.dump(conf, f)
    torch.manual_seed(5)
    return tcnn_fields.TCNNSDF(str(path))


def sphere_loss(sdf_and_gradient, x):
    p = 2.0 * x - 1.0
    sdf, grad = sdf_and_gradient(x)
    world_grad = 0.5 * grad                                     # d sdf / dp
    return ((sdf[:, 0] - (p.norm(dim=-1) - 0.5)) ** 2).mean() + EIK_WEIGHT * ((world_grad.norm(dim=-1) - 1.0) ** 2).mean()


def fit(params, sdf_and_gradient, device, steps=STEPS):
    """-> (held-out loss before, after)"""
    gen = torch.Generator().manual_seed(17)
    held = torch.rand(BATCH, 3, generator=gen).to(device)
    opt = torch.optim.Adam(params, lr=LR)
    first = float(sphere_loss(sdf_and_gradient, held.clone()).detach())
    for _ in range(steps):
        x = torch.rand(BATCH, 3, generator=gen).to(device)
        opt.zero_grad()
        sphere_loss(sdf_and_gradient, x).backward()
        opt.step()
    return first, float(sphere_loss(sdf_and_gradient, held.clone()).detach())


def restated(field):
    """sdf_and_gradient of `field` with the encoding restated in plain torch (CPU)."""
    def f(x):
        x = x.requires_grad_(True)
        sdf = field.sdf_network(O.restate(FIT_CFG, x, field.sdf_encoding.params))[:, :1]
        (grad,) = torch.autograd.grad(sdf.sum(), x, create_graph=True)
        return sdf, grad
    return f


@pytest.mark.gpu
def test_field_fits_a_sphere_with_an_eikonal_term(tmp_path):
    field = make_field(tmp_path / "fit.json").cuda()

    def f(x):
        sdf, _, grad = field.get_all(x, is_training=True)
        return sdf, grad

    first, last = fit(list(field.parameters()), f, torch.device("cuda"))
    print("   sphere fit: held-out loss %.3e -> %.3e (1 / %.0f) in %d steps" % (first, last, first / last, STEPS))
    assert last <= first / 10.0
