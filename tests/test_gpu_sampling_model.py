"""The HIP kernels of the DDGI read side (k_lighting_compose, k_probe_debug, and through them
sampleDDGI and the atlas gather) against the float64 model of the shaders
(tests/ddgi_sampling_model.py) directly, with the bound and the cap of
tests/test_sampling_model.py, and against the oracle bit for bit, on the cases of
tests/sampling_inputs.py. No scene and no update on the device: the atlases go in through
`write`, the c) atlases are the host oracle's.

Tile remap: k_lighting_compose maps workgroups to 64 x 4 tiles by XCD,
tile = (blockIdx & 7) * per + (blockIdx >> 3). 130 x 9 gives 9 tiles, per = 2, 16 workgroups
of which 7 exit; 65 x 5 has partial tiles on both axes; 1 x 1. The output plane is poisoned
with a nonzero, non-NaN fp16 pattern first, so an unwritten tile shows even where 0 is expected.
"""
import numpy as np
import pytest
import torch

from arkoserenderer_amd import abi
from arkoserenderer_amd import ddgi as D
import sampling_inputs as SI
import test_sampling_model as TS

pytestmark = pytest.mark.gpu

POISON = 0x1234  # fp16 0.000757: no colour or alpha of these cases stores it in all four channels


@pytest.fixture(scope="module")
def contexts():
    """One device context per atlas set, filled through `write`."""
    made = {}

    def get(atlas):
        if atlas not in made:
            grid, cfg = (SI.GC, SI.GC_CFG) if atlas == "c" else (SI.G1, SI.G1_CFG)
            ctx = D.DDGIContext(grid, SI.Z_FAR, cfg)
            irr, vis = SI.ATLASES[atlas]()
            ctx.write(abi.ARK_DDGI_ATLAS_IRRADIANCE, irr)
            ctx.write(abi.ARK_DDGI_ATLAS_VISIBILITY, vis)
            made[atlas] = ctx
        return made[atlas]

    yield get
    for ctx in made.values():
        ctx.close()


def device_compose(ctx, case, flags):
    W, H = case["width"], case["height"]
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in case["planes"].items()}
    out = torch.full((H, W, 4), POISON, dtype=torch.int16, device="cuda")
    ctx.lighting_compose(W, H, flags, case["camera"], {k: t.data_ptr() for k, t in dev.items()}, out.data_ptr())
    ctx.synchronize()
    got = out.cpu().numpy().view(np.uint16)
    assert not np.any(np.all(got == POISON, axis=-1)), f"{case['name']}: texels left unwritten"
    return got


def assert_bitwise(what, got, want):
    n = int(np.count_nonzero(got != want))
    assert n == 0, f"{what}: {n} of {got.size} channels differ from the oracle"


@pytest.mark.parametrize("name", list(TS.CASES))
def test_compose_against_model_and_oracle(contexts, name):
    case = TS.CASES[name]
    ctx = contexts(case["atlas"])
    for flags in case["flag_sets"]:
        got = device_compose(ctx, case, flags)
        assert_bitwise(f"{name} flags {flags:#x}", got, TS.oracle_compose(name, flags))
        want, _ = TS.model_compose(name, flags, "float64")
        if case["toleranced"]:
            share = TS.check_within_bound(f"{name} flags {flags:#x} device", got, want, case, flags)
            print(f"{name} flags {flags:#x}: {share:.3%} of the channels outside {TS.ULP_BOUND} fp16 ulps")
        else:  # pixels at probe positions: the class of the result only
            assert np.array_equal((got & 0x7FFF) > 0x7C00, (want & 0x7FFF) > 0x7C00)


@pytest.mark.parametrize("atlas", SI.DEBUG_ATLASES)
def test_probe_debug_against_model_and_oracle(contexts, atlas):
    ctx = contexts(atlas)
    probes, dirs = SI.probe_debug_samples()
    p = torch.from_numpy(probes.astype(np.int32)).cuda()
    d = torch.from_numpy(dirs).cuda()
    node = D.DDGIProbeDebug()
    for mode, scale in SI.DEBUG_MODES:
        node.debug_visualisation, node.distance_scale = mode, scale
        out = torch.full((len(probes), 4), POISON, dtype=torch.int16, device="cuda")
        node.execute(ctx, p, d, out)
        ctx.synchronize()
        got = out.cpu().numpy().view(np.uint16)
        assert_bitwise(f"probe_debug_{atlas} mode {mode}", got, TS.oracle_debug(atlas, mode, scale))
        want = TS.model_debug(atlas, mode, scale, "float64")
        assert np.array_equal(got[:, 3], want[:, 3])
        share = TS.outlier_share(got[:, :3], want[:, :3])
        print(f"probe_debug_{atlas} mode {mode}: {share:.3%} outside {TS.ULP_BOUND} fp16 ulps")
        assert share <= TS.OUTLIER_CAP, (atlas, mode, share)


@pytest.mark.parametrize("size", SI.REMAP_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tile_remap(contexts, size):
    case = SI.remap_case(*size)
    ctx = contexts("a")
    flags = abi.ARK_COMPOSE_DIFFUSE_GI
    got = device_compose(ctx, case, flags)
    want = TS.oracle_for("a").lighting_compose(case["width"], case["height"], flags, case["camera"], case["planes"])
    assert_bitwise(case["name"], got, want)
    model, _ = TS.model_compose(case["name"], flags, "float64", None, size)
    TS.check_within_bound(f"{case['name']} device", got, model, case, flags)
    if case["width"] * case["height"] > 1:
        assert np.count_nonzero(got[..., :3]) > 0
