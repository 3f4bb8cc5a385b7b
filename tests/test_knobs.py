"""CPU: slide_amd/knobs.py declares every SLIDE_* variable once.  Each kind parses a string exactly as the expression it replaced did
(that expression stands beside the expected values, written out), the variables that were read in more than one way still serve every
use, no module of the plan or module path reads the environment itself, the names that tests and tools use are declared, and an
engine keeps the knobs it was built under."""
import glob
import importlib.util
import os
import re

import pytest
import torch

import pair_cases
import tail_cases
import test_plan_merge
from slide_amd import abi, configs, engine as E, knobs, model_spec
from slide_amd.synth import synth_state_dict

CPU = torch.device("cpu")
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
STRINGS = (None, "", "0", "1", "2", "00")  # None: the variable is unset
ERR = ValueError


@pytest.fixture
def env(monkeypatch):
    for k in [k for k in os.environ if k.startswith("SLIDE_") and k not in ("SLIDE_HIP_LIB", "SLIDE_EXPERIMENTS")]:
        monkeypatch.delenv(k)
    return monkeypatch


def _set(env, name, s):
    env.delenv(name, raising=False) if s is None else env.setenv(name, s)


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("plan_digest", os.path.join(ROOT, "tools", "plan_digest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def nets():
    out = {}
    for name, cfg in (("pos", configs.position_ddpm_config()), ("feat", configs.feature_ddpm_config())):
        hp = cfg["pointnet_config"]
        out[name] = hp, synth_state_dict(model_spec.denoiser_param_spec(hp))
    return out


def _engine(nets, net, prec="fp16"):
    return E.DenoiserEngine(*nets[net], 2, CPU, prec=prec)


# one variable of every kind and default shape: (name, the expression that read it before the table, its value for each of STRINGS)
PARSES = [
    ("SLIDE_GLDS", lambda: os.environ.get("SLIDE_GLDS", "1") != "0", (True, True, False, True, True, True)),
    ("SLIDE_SA_CHAIN", lambda: not os.environ.get("SLIDE_SA_CHAIN", "1") == "0", (True, True, False, True, True, True)),
    ("SLIDE_PP", lambda: not os.environ.get("SLIDE_PP", "0") == "0", (False, True, False, True, True, True)),
    ("SLIDE_TWO_LANES", lambda: os.environ.get("SLIDE_TWO_LANES", "0") != "0", (False, True, False, True, True, True)),
    ("SLIDE_TAIL_RX", lambda: os.environ.get("SLIDE_TAIL_RX", "1") != "0", (True, True, False, True, True, True)),
    ("SLIDE_TAIL8", lambda: not os.environ.get("SLIDE_TAIL8", "0") == "0", (False, True, False, True, True, True)),
    ("SLIDE_MODULE_PAIR", lambda: os.environ.get("SLIDE_MODULE_PAIR", "1") != "0", (True, True, False, True, True, True)),
    ("SLIDE_GEMM_CHAIN", lambda: int(os.environ.get("SLIDE_GEMM_CHAIN", "0")), (0, ERR, 0, 1, 2, 0)),
    ("SLIDE_CBW4_TILES", lambda: int(os.environ.get("SLIDE_CBW4_TILES", "1000")), (1000, ERR, 0, 1, 2, 0)),
    ("SLIDE_POS_MULT", lambda: int(os.environ.get("SLIDE_POS_MULT", "2")), (2, ERR, 0, 1, 2, 0)),
    ("SLIDE_STAGGER_US", lambda: float(os.environ.get("SLIDE_STAGGER_US", "0")), (0.0, ERR, 0.0, 1.0, 2.0, 0.0)),
    ("SLIDE_BODY", lambda: os.environ.get("SLIDE_BODY", "0"), ("0", "", "0", "1", "2", "00")),
    ("SLIDE_XS", lambda: os.environ.get("SLIDE_XS", ""), ("", "", "0", "1", "2", "00")),
    ("SLIDE_XS_CBW", lambda: os.environ.get("SLIDE_XS_CBW", "2"), ("2", "", "0", "1", "2", "00")),
    ("SLIDE_GX_N64", lambda: os.environ.get("SLIDE_GX_N64", "1"), ("1", "", "0", "1", "2", "00")),
    ("SLIDE_MODULE_PREC", lambda: os.environ.get("SLIDE_MODULE_PREC", "fp32"), ("fp32", "", "0", "1", "2", "00")),
    ("SLIDE_XS_OCC", lambda: os.environ.get("SLIDE_XS_OCC"), (None, "", "0", "1", "2", "00")),
    ("SLIDE_TAIL_WIDE", lambda: os.environ.get("SLIDE_TAIL_WIDE"), (None, "", "0", "1", "2", "00")),
    ("SLIDE_ABL_DROP", lambda: os.environ.get("SLIDE_ABL_DROP"), (None, "", "0", "1", "2", "00")),
]


def _value(f):
    try:
        return f()
    except ValueError:
        return ERR


@pytest.mark.parametrize("name,before,want", PARSES, ids=[p[0] for p in PARSES])
def test_parse_semantics(env, name, before, want):
    in_snapshot = knobs.KNOBS[name].scope != "live"
    for s, w in zip(STRINGS, want):
        _set(env, name, s)
        got = _value(lambda: knobs.read(name))
        assert got == w and type(got) is type(w) and _value(before) == w, (name, s, got)
        if in_snapshot:
            assert _value(lambda: getattr(knobs.snapshot(), name)) == w, (name, s)
        else:
            assert name not in knobs.Snapshot._fields


def test_every_knob_has_a_kind_a_scope_and_a_parsable_default(env):
    for k in knobs.TABLE:
        assert k.name.startswith("SLIDE_") and k.scope in ("plan", "live", "library") and k.doc
        assert (k.default is None) == (k.kind == "opt"), k.name
        knobs.read(k.name)  # unset: the default parses
    assert set(knobs.Snapshot._fields) == {k.name for k in knobs.TABLE if k.scope in ("plan", "library")}


def _tails(e):
    return [o for o in e.ops if o.kind == abi.OP_ATTN_TAIL]


def test_tail_wide_its_presence_and_its_threshold(env, nets):
    """two uses: set at all, it keeps u / mo chunk-major (_tail_fm); its value is the channel-block count from which a tail runs the wide
    form, 1000 when unset (bit 2 of f[1]).  The feature net's tails have 4, 8 and 16 channel blocks."""
    got = {}
    for s in (None, "1000", "8", "4"):
        _set(env, "SLIDE_TAIL_WIDE", s)
        e = _engine(nets, "feat")
        got[s] = (bool(e._fm), sorted(o.i[5] for o in _tails(e) if int(o.f[1]) & 4), any(int(o.f[1]) & 16 for o in _tails(e)))
    blocks = sorted(o.i[5] for o in _tails(e))
    assert set(blocks) == {4, 8, 16}
    assert got[None] == (True, [], True) and got["1000"] == (False, [], False)
    assert got["8"] == (False, [b for b in blocks if b >= 8], False) and got["4"] == (False, blocks, False)
    env.setenv("SLIDE_TAIL_WIDE", "")
    with pytest.raises(ValueError):  # (as before: present, and no number)
        _engine(nets, "feat")


def test_body_compared_to_0_and_to_2(env, nets):
    """three uses: "0" keeps the three launches per block and fragment-major tails; anything else takes the one-launch body for the
    FP0-sized blocks; "2" for SA0 as well"""
    got = {}
    for s in (None, "0", "1", "2", ""):
        _set(env, "SLIDE_BODY", s)
        e = _engine(nets, "feat")
        got[s] = (sum(o.kind == abi.OP_BLOCK_BODY for o in e.ops), bool(e._fm))
    assert got[None] == got["0"] == (0, True)
    assert got["1"] == got[""] == (1, False) and got["2"] == (2, False)


def test_xs_its_truth_its_levels_and_the_occupancy_cap(env, nets):
    """SLIDE_XS: any value turns chunk-major storage off; "auto" / a list of sample sizes pick the layers of the X-stationary kernel
    (p[10]).  SLIDE_XS_OCC: empty counts as unset; a number n goes into i[9] as 10 + n.  SLIDE_XS_CBW: "4" widens the tiles (i[7])."""
    env.setenv("SLIDE_GX", "0")
    xs = lambda e: [o for o in e.ops if o.kind == abi.OP_GEMM and o.p[10]]
    e = _engine(nets, "feat")
    assert e.use_cm and not xs(e)
    env.setenv("SLIDE_XS", "auto")
    auto = _engine(nets, "feat")
    assert not auto.use_cm and xs(auto) and {o.i[9] for o in xs(auto)} == {0} and {o.i[7] for o in xs(auto)} == {2}
    assert {o.i[4] for o in xs(auto)} == {7, 8}
    env.setenv("SLIDE_XS", "7")
    only7 = _engine(nets, "feat")
    assert not only7.use_cm and {o.i[4] for o in xs(only7)} == {7}
    env.setenv("SLIDE_XS", "auto")
    env.setenv("SLIDE_XS_OCC", "")
    assert {o.i[9] for o in xs(_engine(nets, "feat"))} == {0}
    env.setenv("SLIDE_XS_OCC", "2")
    env.setenv("SLIDE_XS_CBW", "4")
    capped = _engine(nets, "feat")
    assert {o.i[9] for o in xs(capped)} == {12} and 4 in {o.i[7] for o in xs(capped)}
    assert {o.i[9] for o in capped.ops if o.kind == abi.OP_GEMM and not o.p[10]} == {0}


def test_no_environment_reads_outside_the_table():
    for f in ("engine.py", "diffusion.py", "rows.py", "nn_ops.py"):
        src = open(os.path.join(ROOT, "slide_amd", f)).read()
        assert "os.environ" not in src and "getenv" not in src, f


def test_library_scope_is_what_the_library_reads():
    found = set()
    for f in glob.glob(os.path.join(ROOT, "slide_amd", "csrc", "**", "*"), recursive=True):
        if os.path.isfile(f) and f.endswith((".hip", ".h", ".cpp", ".hpp", ".c")):
            found |= set(re.findall(r'getenv\("(SLIDE_\w+)"\)', open(f).read()))
    assert found and found == {k.name for k in knobs.TABLE if k.scope == "library"}


def test_knob_names_of_tests_and_tools_are_declared(tool):
    used = {kv.split("=")[0] for ks in tool.KNOBS for kv in ks.split()}
    used |= {k for d in test_plan_merge.KNOBS for k in d}
    used |= {k for c in list(pair_cases.CASES) + list(tail_cases.CASES) for k in c["env"]}
    assert len(used) > 30 and used <= set(knobs.KNOBS), sorted(used - set(knobs.KNOBS))
    # ... and the digest matrix leaves no plan knob of the engine at its default everywhere
    emitted = set(re.findall(r"\bk(?:nobs)?\.(SLIDE_\w+)", open(os.path.join(ROOT, "slide_amd", "engine.py")).read()))
    in_matrix = {kv.split("=")[0] for ks in tool.KNOBS for kv in ks.split()}
    assert len(emitted) >= 40 and emitted <= in_matrix, sorted(emitted - in_matrix)


def test_an_engine_keeps_the_knobs_it_was_built_under(env, nets, tool):
    e = _engine(nets, "pos")
    before, d0 = e.knobs, tool.plan_digest(e)[0]
    assert before == knobs.snapshot() and before.SLIDE_PACKED_VECS is True
    env.setenv("SLIDE_PACKED_VECS", "0")
    assert e.knobs is before and e.knobs.SLIDE_PACKED_VECS is True
    with pytest.raises(AttributeError):
        e.knobs.SLIDE_PACKED_VECS = False
    e2 = _engine(nets, "pos")
    assert e2.knobs != before and e2.knobs.SLIDE_PACKED_VECS is False and tool.plan_digest(e2)[0] != d0


def test_bare_builders_pin_the_derived_attributes_and_see_the_rest(env):
    env.setenv("SLIDE_GLDS", "0")
    env.setenv("SLIDE_GLDS_WIDE", "2")
    env.setenv("SLIDE_PERSISTENT", "1")
    env.setenv("SLIDE_TWO_LANES", "1")
    env.setenv("SLIDE_GX_N64", "0")
    m = E.DenoiserEngine.__new__(E.DenoiserEngine)
    m._plan_state(2, CPU, "fp16")
    assert (m.use_glds, m.glds_nst, m.persistent, m.two_lanes) == (True, 0, 0, False)
    assert (m.use_cm, m.use_gx, m.use_gxs) == (False, False, False)
    assert m.knobs.SLIDE_GLDS is False and m.knobs.SLIDE_GX_N64 == "0" and m.knobs.SLIDE_PERSISTENT == 1
