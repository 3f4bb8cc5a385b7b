"""CPU: tools/plan_digest.py, the address-free digest of a built plan that refactors of the plan builder are checked with, sees what it
must: it is stable, it changes with one ulp of one weight and with one knob, and a segment described by plain tuples packs to the
same bytes as one described by the engine's named records."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from slide_amd import configs, engine as E, model_spec
from slide_amd.synth import synth_state_dict

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def tool():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "plan_digest.py")
    spec = importlib.util.spec_from_file_location("plan_digest", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def net():
    hp = configs.position_ddpm_config()["pointnet_config"]
    return hp, synth_state_dict(model_spec.denoiser_param_spec(hp))


@pytest.fixture
def no_knobs(monkeypatch):
    for k in [k for k in os.environ if k.startswith("SLIDE_") and k not in ("SLIDE_HIP_LIB", "SLIDE_EXPERIMENTS")]:
        monkeypatch.delenv(k)
    return monkeypatch


def _digest(tool, hp, sd):
    d, unresolved = tool.plan_digest(E.DenoiserEngine(hp, sd, 2, CPU, prec="fp16"))
    assert unresolved == 0
    return d


def test_digest_is_stable_and_sees_one_ulp_and_one_knob(tool, net, no_knobs):
    hp, sd = net
    base = _digest(tool, hp, sd)
    assert _digest(tool, hp, sd) == base
    name = "SA_modules.0.mlps.0.second_mlp.0.bias"
    sd2 = dict(sd)
    sd2[name] = sd[name].copy()
    sd2[name][3] = np.nextafter(sd[name][3], np.float32(np.inf))
    assert sd2[name][3] != sd[name][3] and _digest(tool, hp, sd2) != base
    no_knobs.setenv("SLIDE_PACKED_VECS", "0")
    assert _digest(tool, hp, sd) != base


def _bare_layers(records):
    """two launches through _gemm on a bare builder (16-row samples, 32 rows), every tuple of the segments and of the call either
    plain or one of the engine's records"""
    rs = np.random.RandomState(7)
    f = lambda *shape: rs.standard_normal(shape).astype(np.float32)
    as_ = (lambda T, *v: T(*v)) if records else (lambda T, *v: v)
    m = E.DenoiserEngine.__new__(E.DenoiserEngine)
    m._plan_state(2, CPU, "fp32")
    rows, K_in, N = 32, 64, 96
    lay = E.gn_layout(N)  # groups of 3 in runs of 4: a permuted layout, 128 physical channels
    Np = E.ru(lay[1])
    X, idx = m.A.put(f(rows, K_in)), m.A.put(np.array([1], np.int32))
    norm = dict(w=f(N, K_in), bias=f(N), mode=E.EPI_NORM, flags=E.F_POST_RELU, gn=(f(lay[2] * lay[4] // lay[3]), f(lay[2] * lay[4] // lay[3])),
                layout=lay if records else tuple(lay), out=m._buf(rows, Np),
                addvec=as_(E.AddVec, m.A.put(f(4, 2 * Np)), 0, Np, idx, 2 * Np), pre_add=as_(E.PreAdd, m.A.put(f(rows, Np)), 0))
    stat = dict(w=f(32, K_in), mode=E.EPI_STATS, flags=E.F_PRE_RELU, out=m._buf(rows, 64), out_coff=32,
                stats=as_(E.Stats, m.A.zeros(2, 64), m.A.zeros(2, 64), 32, 16.0), pre_add=as_(E.PreAdd, m.A.put(f(2, 96)), 4, 64))
    m._gemm(X, 4, [norm, stat], in_affine=as_(E.InAffine, m.A.put(f(2, 2 * K_in)), m.A.put(f(2, 2 * K_in)), K_in, 2 * K_in))
    nbr = m.A.put(rs.randint(0, 16, (rows, 16)).astype(np.int32))
    m._gemm(m.A.put(f(rows, 32)), 4, [dict(w=f(32, 96), bias=f(32), out=m._buf(rows, 32))], gather=as_(E.Gather, m.A.put(f(rows, 64)), nbr, 16, 2))
    return m


def test_plain_tuples_and_records_pack_the_same(tool, no_knobs):
    (a, ua), (b, ub) = (tool.plan_digest(_bare_layers(r)) for r in (False, True))
    assert ua == 0 and ub == 0 and a == b
    assert len(_bare_layers(True).plan) == 2
