"""The `small` scene of tests/golden/scenes.py with its body voxelised at ANISO = (0.004, 0.005, 0.008) (dhw): three different voxel
sizes, and with the 0.3 x 0.5 x 0.2 m body three different out_sh entries, so that every place that decides by hand which entry of
voxel_size belongs to which axis shows in the result.  Shared by tests/test_aniso_cases_host.py (the oracle alone: the scene tells
ANISO from its reverse) and tests/test_gpu_aniso_voxels.py (every consumer of the grid against the oracle at ANISO).  CPU only."""
import functools

from tests.voxelize_cases import ANISO  # noqa: F401

SCENE = "small"


@functools.lru_cache(maxsize=None)
def scene():
    """-> dict(recipe, sd, body, batch, sdt, vols (the oracle's fp32 volumes, NCDHW), out_sh): computed once, never written to."""
    from tests import helpers as H
    from tests.golden import scenes

    r, sd, body, batch, cam, t_rand = scenes.build(SCENE, ANISO)
    assert t_rand is None and r["mode"] == "train"
    sdt, vols, out_sh = H.oracle_volumes(sd, batch, True)
    assert len(set(out_sh)) == 3, out_sh
    return dict(recipe=r, sd=sd, body=body, batch=batch, sdt=sdt, vols=vols, out_sh=out_sh)


@functools.lru_cache(maxsize=None)
def oracle_render(voxel_size=ANISO):
    """orc.render of the scene on its own volumes with the grid coordinates formed at `voxel_size` -> dict of numpy arrays."""
    import torch

    from oracle import neuralbody_oracle as orc

    s = scene()
    with torch.no_grad():
        out = orc.render(s["sdt"], s["batch"], n_samples=s["recipe"]["n_samples"], voxel_size=tuple(voxel_size), training=True,
                         white_bkgd=s["recipe"]["white_bkgd"], feature_volume=s["vols"])
    return {k: v.numpy() for k, v in out.items()}
