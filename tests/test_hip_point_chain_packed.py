"""SLIDE_OP_POINT_CHAIN in its PACKED form (SlidePointChainArgs.wpk_bytes: every weight in one buffer of MFMA fragments,
slide_amd/chain_pack.py) against the row-major form of the SAME hand-built arguments, BITWISE: the packed launch reads the same fp16
values into the same registers and runs the same arithmetic, so eps and the written X columns must agree bit for bit.  The row-major
form is held to the float64 reference at derived bounds by tests/test_hip_point_chain.py; equality to it is the whole bound here.

  equality        every dense case of tests/chain_cases.py in both forms (fp16, WIDE): rows 16 (one sample, the workgroup's second a
                  clamp), 48 (two workgroups, the last half full), 32, 112; kz 32 / 96 / 192; n1c 1 / 2; a per-timestep table, per-sample
                  t rows, no t rows; with and without the class rows; what the launch does not own keeps its sentinel
  hand-over       the fused update rides on the packed launch too: three unsynchronised launches (eagerly, and as one captured graph
                  replayed three times) leave the state, the timestep block and eps of the row-major launches
  refusals        -3 and nothing launched for a size that fits another n1c / another kz / neither form, a misaligned buffer, a
                  row-major or *_lo pointer left set beside the packed one"""
import numpy as np
import pytest

import chain_cases as cc
import test_hip_point_chain as rm
import update_cases as uc
from op_harness import SENTINEL, Dev, bits, run, status

F32, F16 = np.float32, np.float16
DENSE = [c["name"] for c in cc.CASES if not c["probe"]]


def _pack_into(ch, d, form):
    """turns the row-major arguments of a _Chain into the packed form (the same fp16 values, packed once on the host)"""
    from slide_amd import chain_pack
    parts = [cc.split(d[k]) for k in ("Wz", "W2", "W0", "W1")]
    buf = chain_pack.pack(*[hi.astype(F16) for hi, _ in parts], [lo.astype(F16) for _, lo in parts] if form == "wide" else None)
    a = ch.args
    a.Wz, a.wpk_bytes = ch.dev.put(buf).data_ptr(), buf.size * 2
    a.W2 = a.W0 = a.W1 = a.Wz_lo = a.W2_lo = a.W0_lo = a.W1_lo = None
    return ch


@pytest.mark.gpu
@pytest.mark.parametrize("form", cc.FORMS)
@pytest.mark.parametrize("name", DENSE)
def test_packed_launch_is_bitwise_the_row_major_launch(gpu_device, name, form):
    c = cc.CASE_BY_NAME[name]
    d = rm._ref(name, form)[0]
    outs = []
    for packed in (False, True):
        ch = rm._Chain(gpu_device, c, d, form)
        if packed:
            _pack_into(ch, d, form)
        run([ch.op()])
        ch.check_poison()
        X, eps, _ = ch.outputs()
        outs.append((X[:c["rows"], :128], eps))
    assert (bits(outs[0][1]) == bits(outs[1][1])).all(), "eps: max |diff| %g" % np.abs(outs[0][1] - outs[1][1]).max()
    assert (bits(outs[0][0]) == bits(outs[1][0])).all(), "X[:, :128] differs"


@pytest.mark.gpu
@pytest.mark.parametrize("graph", (False, True), ids=("eager", "graph"))
@pytest.mark.parametrize("name,C", [("r16_kz96_gnmean", 51), ("r112_kz192_pad", 19)], ids=("one_workgroup", "four_workgroups"))
def test_packed_fused_hand_over_three_launches(gpu_device, name, C, graph):
    """fuse_update takes the packed form: three launches back to back, each reading the t row its predecessor handed over"""
    c = cc.CASE_BY_NAME[name]
    assert c["tvec"] == "shared"
    d = rm._ref(name, "wide")[0]
    npts = c["rows"]
    x, kp, _, _ = rm._feat_inputs(npts, C, False, seed=npts + C + 2)
    tabs = uc.feat_tables()
    noise = np.random.RandomState(8).standard_normal((rm.LAUNCHES, npts * C)).astype(F32)
    got = []
    for packed in (False, True):
        ch = rm._Chain(gpu_device, c, d, "wide", t_dev=Dev(gpu_device).t_dev(rm.T0, 0))
        if packed:
            _pack_into(ch, d, "wide")
        dx = rm._fuse(ch, C, x, kp, tabs, 1.5, noise=noise)
        run([ch.op()], times=rm.LAUNCHES, graph=graph)
        got.append((dx.cpu().numpy(), ch.t_dev.cpu().numpy().tolist(), ch.outputs()[1]))
    assert got[1][1][:3] == [rm.T0 - rm.LAUNCHES, rm.LAUNCHES, 0] and got[0][1] == got[1][1]
    assert (bits(got[0][0]) == bits(got[1][0])).all(), "the state after three fused launches differs"
    assert (bits(got[0][2]) == bits(got[1][2])).all(), "eps of the last launch differs"
    assert not (got[1][0] == x).all()  # (the launches did update the state)


@pytest.mark.gpu
@pytest.mark.parametrize("what", ("bytes_of_n1c_2", "bytes_of_kz_64", "bytes_plus_1k", "bytes_between_forms", "negative", "misaligned",
                                  "w2_left_set", "lo_left_set"))
def test_launcher_refuses_inconsistent_packed_arguments(gpu_device, what):
    from slide_amd import chain_pack
    c = cc.CASE_BY_NAME["r16_kz32"]  # kz 32, k0 160, n1c 1
    d = rm._ref("r16_kz32", "wide")[0]
    ch = rm._Chain(gpu_device, c, d, "wide")
    keep = ch.args.W2, ch.args.W0_lo
    a = _pack_into(ch, d, "wide").args
    spare = ch.dev.put(np.zeros(1 << 16, F16))  # (the pointer a refused launch would have read stays inside an allocation)
    if what == "bytes_of_n1c_2":
        a.wpk_bytes = 1024 * chain_pack.n_fragments(32, 160, 2, True)
    elif what == "bytes_of_kz_64":
        a.wpk_bytes = 1024 * chain_pack.n_fragments(64, 160, 1, True)
    elif what == "bytes_plus_1k":
        a.wpk_bytes += 1024
    elif what == "bytes_between_forms":
        a.wpk_bytes = a.wpk_bytes * 3 // 4
    elif what == "negative":
        a.wpk_bytes = -a.wpk_bytes
    elif what == "misaligned":
        a.Wz = spare.data_ptr() + 8
    elif what == "w2_left_set":
        a.W2 = keep[0]
    else:
        a.W0_lo = keep[1]
    assert status(ch.op()) == -3 * 1000  # (slide_run_ops: status * 1000 - index of the failing op)
    X, eps, tail = ch.outputs()
    assert (eps == F32(SENTINEL)).all() and (tail == F32(SENTINEL)).all() and (X[:, :128] == F16(SENTINEL)).all(), "a kernel ran"
