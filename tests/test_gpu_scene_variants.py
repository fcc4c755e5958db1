"""Parity off the default scene: the HIP kernels against the CPU oracle on the scene variants of
tests/scene_variants.py (physics, solver, reset and bounds parameters the other GPU tests leave at their
defaults) and on the pile-up (poles thrown against each other: merged solves in every env, pole-pole2
contacts of every branch kind, contact-cap overflow in every env), through the C-ABI.

Every comparison is on raw bits; there are no tolerances.  The contact-cap overflow counters are compared
against the oracle's wherever the state is.  The oracle's side of each run is computed once
(scene_variants.variant_run / pileup_run) and shared between the kernel shapes;
tests/test_scene_variants_cpu.py pins its preconditions (finite, the variant took effect, the pile-up's
coverage), so a failure here is a parity failure."""
import numpy as np
import pytest
import torch

from cartpoleplusplus_amd import abi
from tests import scene_variants as SV
from tests.test_gpu_parity import SHAPE_IDS, SHAPES, _assert_same, _np, _pair

pytestmark = pytest.mark.gpu

# one shape per kernel family: throughput, two-lane latency, 16 lanes per env (one env per wave on reset), and the
# reset list tiered by its length
FAMILY = [("throughput", "throughput"), ("latency", "latency"), ("wide", "wide64"), ("throughput", "list")]
FAMILY_IDS = ["tp-tp", "lat-lat", "wide-wide64", "tp-list"]


def _bits(a):
    """A float64 array as its uint64 bits (so that -0.0 != +0.0, as _assert_same does for float32)."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _handle(O, run, shape, mutate, precision="f32", **kw):
    gpu, _ = _pair(O, shape, mutate=mutate, precision=precision, oracle=False, **kw)
    assert bytes(gpu.cfg) == bytes(run["cfg"]), "the recorded oracle run is of another config"
    return gpu


def _compare_end(gpu, rec, what):
    """State SoA, episode returns and lengths, overflow and nonfinite counters against a drive() checkpoint."""
    _assert_same(_bits(_np(gpu.get_state())), _bits(rec["state"]), what + " state")
    ret, length = gpu.episode_returns()
    _assert_same(_np(ret), rec["returns"], what + " episode returns")
    _assert_same(_np(length), rec["lengths"], what + " episode lengths")
    _assert_same(_np(gpu.overflow_counts()), rec["overflow"], what + " overflow counts")
    _assert_same(_np(gpu.nonfinite_counts()), rec["nonfinite"], what + " nonfinite counts")


def _step_through(gpu, run, steps, what, terminal=True):
    for t in range(steps):
        go, gr, gd = gpu.step(torch.from_numpy(run["actions"][t]).cuda())
        _assert_same(_np(go), run["obs"][t], f"{what}: obs step {t}")
        _assert_same(_np(gr), run["reward"][t], f"{what}: reward step {t}")
        _assert_same(_np(gd), run["done"][t], f"{what}: done step {t}")
        if terminal:
            done = run["done"][t].astype(bool)
            _assert_same(_np(gpu.terminal_obs)[done], run["term"][t][done], f"{what}: terminal obs step {t}")


def _reset_and_compare(gpu, run, what):
    _assert_same(_np(gpu.reset()), run["reset_obs"], what + ": reset obs")
    _assert_same(_bits(_np(gpu.get_state())), _bits(run["reset_state"]), what + ": reset state")
    _assert_same(_np(gpu.overflow_counts()), run["reset_overflow"], what + ": reset overflow counts")


@pytest.mark.parametrize("shape", FAMILY, ids=FAMILY_IDS)
@pytest.mark.parametrize("name", SV.NAMES)
def test_variant_step_parity(oracle_mod, name, shape):
    """The measured run of every variant (B = 64, R = 2, F_init 55, autoreset, bounds termination, episodes
    of at most 70 steps, 100 steps of random discrete actions) on one shape per kernel family."""
    run = SV.variant_run(oracle_mod, name)
    gpu = _handle(oracle_mod, run, shape, SV.VARIANTS[name], **SV.RUN)
    _reset_and_compare(gpu, run, name)
    _step_through(gpu, run, SV.RUN_STEPS, name)
    _compare_end(gpu, run["at"][SV.RUN_STEPS], name)
    gpu.close()


@pytest.mark.parametrize("name", SV.NAMES)
def test_variant_f64(oracle_mod, name):
    """Every variant on an fp64 handle against the fp64 oracle, 60 steps; the state as uint64 bits."""
    run = SV.variant_run(oracle_mod, name, "f64")
    gpu = _handle(oracle_mod, run, None, SV.VARIANTS[name], precision="f64", **SV.RUN)
    assert gpu.get_state().dtype == torch.float64
    _reset_and_compare(gpu, run, name)
    _step_through(gpu, run, 60, name + " f64")
    _compare_end(gpu, run["at"][60], name + " f64")
    gpu.close()


@pytest.mark.parametrize("shape", [("throughput", "throughput"), ("wide", "wide")], ids=["tp-tp", "wide-wide"])
@pytest.mark.parametrize("name", ["allfric", "nofric", "it7", "squat", "reset"])
def test_variant_rollout(oracle_mod, name, shape):
    """cp_rollout, K = 60 in one launch: the rollout kernel has its own inline reset, so settle_steps and
    initial_force_steps (variant reset) and the friction / solver routing matter there once more."""
    K = 60
    run = SV.variant_run(oracle_mod, name)
    gpu = _handle(oracle_mod, run, shape, SV.VARIANTS[name], **SV.RUN)
    _reset_and_compare(gpu, run, name)
    go, gr, gd = gpu.rollout(torch.from_numpy(run["actions"][:K]).cuda())
    _assert_same(_np(gd), run["done"][:K], name + " rollout: done")
    _assert_same(_np(gr), run["reward"][:K], name + " rollout: reward")
    _assert_same(_np(go), run["obs"][:K], name + " rollout: obs")
    done = run["done"][:K].astype(bool)
    _assert_same(_np(gpu.rollout_terminal_obs)[done], run["term"][:K][done], name + " rollout: terminal obs")
    _compare_end(gpu, run["at"][K], name + " rollout")
    gpu.close()


@pytest.mark.parametrize("shape", [("throughput", "list"), ("latency", "latency")], ids=["tp-list", "lat-lat"])
@pytest.mark.parametrize("name", ["allfric", "bounds", "reset"])
def test_variant_next_step(oracle_mod, name, shape):
    """CP_AUTORESET_NEXT_STEP: the reset of a finishing env runs on the library's stream beside the next
    step kernel, on the variant's scene."""
    run = SV.variant_run(oracle_mod, name, autoreset=abi.CP_AUTORESET_NEXT_STEP)
    gpu = _handle(oracle_mod, run, shape, SV.VARIANTS[name], **{**SV.RUN, "autoreset": abi.CP_AUTORESET_NEXT_STEP})
    _reset_and_compare(gpu, run, name)
    _step_through(gpu, run, SV.RUN_STEPS, name + " next_step")
    _compare_end(gpu, run["at"][SV.RUN_STEPS], name + " next_step")
    assert run["done"].any()
    gpu.close()


def _pileup(gpu, run, what):
    gpu.reset()
    gpu.set_state(torch.from_numpy(run["start"]).cuda())
    _assert_same(_bits(_np(gpu.get_state())), _bits(run["start"]), what + ": placed state")
    T = len(run["actions"])
    _step_through(gpu, run, T, what, terminal=False)
    _compare_end(gpu, run["at"][T], what)
    assert run["at"][T]["overflow"].any()


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("cart_friction", SV.PILEUP_CART_FRICTION, ids=["cartmu0", "cartmu0.4"])
def test_pileup(oracle_mod, cart_friction, shape):
    """Poles thrown against each other (B = 96, R = 3): every env runs merged solves, pole-pole2 (global
    pair 8) touches in most envs on faces of A, faces of B and edges, and every env overflows the contact
    caps, so the truncated-manifold paths (m < cnt, fcnt < cnt) run under the overflow comparison.  With
    cart friction 0.4 the cross pairs 5-7 carry friction rows too.  Measured on the fp32 oracle (cart
    friction 0 / 0.4): merged substeps 18,447 / 16,406, pole-pole2 contacts in 87 / 80 envs, overflow in
    96 / 96 envs, 24,041 / 235,242 dropped rows."""
    run = SV.pileup_run(oracle_mod, cart_friction)
    gpu = _handle(oracle_mod, run, shape, lambda c: SV.pileup_config(c, cart_friction), **SV.PILEUP)
    _pileup(gpu, run, f"pile-up mu {cart_friction}")
    gpu.close()


@pytest.mark.parametrize("cart_friction", SV.PILEUP_CART_FRICTION, ids=["cartmu0", "cartmu0.4"])
def test_pileup_f64(oracle_mod, cart_friction):
    run = SV.pileup_run(oracle_mod, cart_friction, "f64")
    gpu = _handle(oracle_mod, run, None, lambda c: SV.pileup_config(c, cart_friction), precision="f64", **SV.PILEUP)
    _pileup(gpu, run, f"pile-up f64 mu {cart_friction}")
    gpu.close()
