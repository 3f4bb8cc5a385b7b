"""CPU: the plan's launch records (engine.Launch), the one rewrite driver the merge passes share, and the tables derived from the
finished launch list -- on synthetic launch lists, then as invariants of real plans over the knob matrix (built on the CPU device)."""
import pytest
import torch

from slide_amd import configs, engine as E, model_spec
from slide_amd.synth import synth_state_dict


def _plan(*specs):
    """launches of kind OP_GEMM with i[0] = position; spec = (flops, nbytes, name, roles)"""
    return [E.Launch(E.make_op(E.OP_GEMM, i=(k,)), *s) for k, s in enumerate(specs)]


def _merge_at(first, n, kind=E.OP_GEMM_CHAIN, name="merged"):
    def match(plan, i):
        if plan[i].op.i[0] == first:
            return n, [(E.make_op(kind), name, plan[i:i + n])]
    return match


def test_pair_and_run_merges_sum_the_accounting():
    plan = _plan((10, (1, 2), "a", ()), (20, (3, 4), "b", ()), (None, None, None, ()), (5, None, "d", ()), (7, (1, 1), None, ()))
    out = E.rewrite(plan, _merge_at(0, 2))
    assert len(out) == 4 and out[0].op.kind == E.OP_GEMM_CHAIN
    assert (out[0].flops, out[0].nbytes, out[0].name) == (30, (4, 6), "merged")
    assert out[1:] == plan[2:]  # unmatched launches are the same objects
    out = E.rewrite(plan, _merge_at(1, 4, name="run"))
    assert len(out) == 2 and out[0] is plan[0]
    assert (out[1].flops, out[1].nbytes, out[1].name) == (32, (4, 5), "run")  # (nothing recorded counts as zero)


def test_unmatched_launches_carry_their_accounting():
    plan = _plan((10, (1, 2), "a", ()), (None, (3, 4), None, ()), (0, None, "c", ()), (None, None, None, ()))
    out = E.rewrite(plan, lambda plan, i: None)
    assert out == plan
    t = E.plan_tables(out)
    assert t["gemm_flops"] == {0: 10, 2: 0} and t["gemm_bytes"] == {0: (1, 2), 1: (3, 4)} and t["kernel_names"] == {0: "a", 2: "c"}
    assert [o.i[0] for o in t["ops"]] == [0, 1, 2, 3]
    # a merge in front shifts every later position
    t = E.plan_tables(E.rewrite(plan, _merge_at(0, 2)))
    assert t["gemm_flops"] == {0: 10, 1: 0} and t["gemm_bytes"] == {0: (4, 6)} and t["kernel_names"] == {0: "merged", 1: "c"}


def test_a_replacement_may_keep_launches_between_the_merged_ones():
    plan = _plan((1, (1, 0), "p", ("x",)), (2, (2, 0), "gx", ("y",)), (4, (4, 0), "chain", ("z",)), (8, None, None, ()))

    def match(plan, i):  # [p, gx, chain] -> [chain + p, gx]
        if i == 0:
            return 3, [(E.make_op(E.OP_SA_CHAIN_P), "chain_p", [plan[0], plan[2]]), plan[1]]
    out = E.rewrite(plan, match)
    assert [e.name for e in out] == ["chain_p", "gx", None] and out[1] is plan[1] and out[2] is plan[3]
    assert (out[0].flops, out[0].nbytes, out[0].roles) == (5, (5, 0), {"x", "z"})


def test_roles_follow_their_launches():
    plan = _plan((1, None, None, ("prep",)), (1, None, None, ()), (1, None, None, ()), (1, None, None, ("xyz_copy",)),
                 (1, None, None, ("head0",)), (1, None, None, ("head1",)), (1, None, None, ("xyz_copy",)), (1, None, None, ("eps_copy",)))
    t = E.plan_tables(plan)
    assert (t["prep_idx"], t["xyz_copy_idx"], t["head"], t["eps_copy_idx"], t["point_chain"]) == (0, [3, 6], [4, 5], 7, None)
    t = E.plan_tables(E.rewrite(plan, _merge_at(1, 2)))
    assert (t["prep_idx"], t["xyz_copy_idx"], t["head"], t["eps_copy_idx"]) == (0, [2, 5], [3, 4], 6)
    t = E.plan_tables(E.rewrite(plan, _merge_at(0, 2)))  # the merged launch has the union of the roles
    assert (t["prep_idx"], t["xyz_copy_idx"], t["head"], t["eps_copy_idx"]) == (0, [2, 5], [3, 4], 6)


def test_head_roles_on_one_launch_derive_no_head():
    plan = _plan((1, None, None, ()), (1, None, None, ("head0",)), (1, None, None, ("head1",)), (1, None, None, ("eps_copy",)))
    assert E.plan_tables(plan)["head"] == [1, 2]
    t = E.plan_tables(E.rewrite(plan, _merge_at(1, 2)))
    assert t["head"] is None and t["eps_copy_idx"] == 2
    assert E.plan_tables(E.rewrite(plan, _merge_at(0, 2)))["head"] == [0, 1]  # merged with a launch in front: still two launches


def test_point_chain_roles_must_stay_on_four_consecutive_launches():
    roles = [(), ("pc0",), ("pc1",), ("pc2", "head0"), ("pc3", "head1"), ("eps_copy",)]
    plan = _plan(*[(1, None, None, r) for r in roles])
    assert E.plan_tables(plan)["point_chain"] == [1, 2, 3, 4]
    assert E.plan_tables(E.rewrite(plan, _merge_at(0, 2)))["point_chain"] == [0, 1, 2, 3]
    assert E.plan_tables(E.rewrite(plan, _merge_at(2, 2)))["point_chain"] is None  # two layers in one launch
    assert E.plan_tables(E.rewrite(plan, _merge_at(1, 4)))["point_chain"] is None
    apart = plan[:3] + _plan((1, None, None, ())) + plan[3:]  # a launch between the layers
    t = E.plan_tables(apart)
    assert t["point_chain"] is None and t["head"] == [4, 5]
    assert E.plan_tables(plan[:4] + plan[5:])["point_chain"] is None  # a layer missing


# ------------------------------------------------------------------------------------------------------------ real plans
KNOBS = [{}, {"SLIDE_GEMM_CHAIN": "256"}, {"SLIDE_GEMM_CHAIN": "100000"}, {"SLIDE_GX_DUAL": "0"}, {"SLIDE_CHAIN_P": "0"}, {"SLIDE_PP": "1"},
         {"SLIDE_FOLD_COPIES": "0"}, {"SLIDE_SA_CHAIN": "0"}, {"SLIDE_GXS_CHAIN": "0", "SLIDE_GX_DUAL": "0"}, {"SLIDE_MERGE_Q": "0"},
         {"SLIDE_POINT_CHAIN": "0"}, {"SLIDE_TWO_LANES": "1"}]
NAMED = (("sa_chain_p", E.OP_SA_CHAIN_P), ("dual", E.OP_GEMM_GX_DUAL), ("gemm_chain_kernel", E.OP_GEMM_CHAIN),
         ("pp_stage_kernel", E.OP_PP_STAGE), ("attn_tail_split_kernel", E.OP_ATTN_TAIL))


@pytest.fixture(scope="module")
def nets():
    out = {}
    for net, cfg in (("pos", configs.position_ddpm_config()), ("feat", configs.feature_ddpm_config())):
        hp = cfg["pointnet_config"]
        out[net] = (hp, synth_state_dict(model_spec.denoiser_param_spec(hp)))
    return out


def test_a_bare_builder_drives_one_sa_block_through_records(nets, monkeypatch):
    """the block planner's phases (_attn_open -> _attn_scores -> the Mlp tail -> _attn_finish) on a bare builder, over the state dict of
    the position net's first SA block (its widths, 32 and 64 channels, are the smallest the emitters take): the launches are the ones
    the full plan has for that block, the emitters leave no attribute behind on the engine, and what the phases hand over are complete
    records"""
    for k in {k for ks in KNOBS for k in ks}:
        monkeypatch.delenv(k, raising=False)
    hp, sd = nets["pos"]
    B, C, mp, ap = 2, 3, "SA_modules.0.mlps.0", "SA_modules.0.attention_modules.0"
    full = E.DenoiserEngine(hp, sd, B, torch.device("cpu"), prec="fp16")
    kinds = [e.op.kind for e in full.plan]
    k0, k1 = kinds.index(E.OP_PREP_POINTS) + 1, kinds.index(E.OP_ATTN_TAIL) + 1
    assert kinds[k0] == E.OP_PAIR_FIRST and E.OP_PAIR_FIRST not in kinds[k0 + 1:k1]  # (one block)

    m = E.DenoiserEngine.__new__(E.DenoiserEngine)
    m._plan_state(B, torch.device("cpu"), "fp16")
    m.use_cm = m.use_gx = True
    m.use_gxs = False
    m._cm, m._fm, m._cm_copy, m._tail_of, m._tvec, m._cvec = set(), set(), {}, {}, [], []
    m.sd = {k: torch.as_tensor(v).detach().numpy().astype("float32") for k, v in sd.items() if k.startswith("SA_modules.0.")}
    m._n_fc = m._t_bs = m.sd[mp + ".fc.weight"].shape[0]
    m._c_bs = m.sd[mp + ".fc_condition.weight"].shape[0]
    m.xyz, m.tvec, m.cvec = m.A.zeros(B * 16, 3), m.A.zeros(B, m._n_fc), m.A.zeros(B, m._c_bs)
    m._chain_keep, m._dual_keep, m._chain_p_keep, m._pp_keep = [], [], [], []
    before = set(vars(m))

    c_last = m.sd[mp + ".res_connect.weight"].shape[0]
    feat, out = m._buf(B * 16, C), m._buf(B * 16, c_last)
    mo = m._buf(B * 256, c_last, cm=True, fm=m._tail_fm(mp, ap, 8, c_last))
    first, res = m._mlp_segments(mp, m.tvec, None, None)
    opened = m._attn_open(ap, 8, feat, mo, first, res, pair=(feat, C, dict(rel=C, abs=C + 3, ctr=C + 6)))
    st = m._attn_scores(opened)
    m._mlp_tail(mp, 8, None, m.cvec, None, mo, pair=st.pair)
    m._attn_finish(st, out)
    for merge in (m._merge_chains, m._merge_gx_pairs, m._merge_chain_query, m._merge_pp):  # (the passes _build runs, in its order)
        m.plan = E.rewrite(m.plan, merge())

    assert [e.op.kind for e in m.plan] == kinds[k0:k1]
    assert [e.name for e in m.plan] == [e.name for e in full.plan[k0:k1]]
    assert set(vars(m)) == before
    assert m._tvec == [(mp + ".fc", m._n_fc)] and m._cvec == [(mp + ".fc_condition", m._c_bs)]
    assert opened.end == st.end == "fused" and opened.P is None and opened.u is None and st.P is not None and st.u is not None and st.S is None
    assert opened[:-4] == st[:-4]  # (the score phase fills in its own fields and nothing else)
    for r, T in ((opened, E.AttnState), (st, E.AttnState), (st.pair, E.BlockPair), (st.pair.t, E.PairTables), (st.lay, E.GnLayout),
                 (st.pair.lay1, E.GnLayout), (st.pair.add1, E.AddVec)):
        assert type(r) is T and isinstance(r, tuple) and len(r) == len(T._fields) and not hasattr(r, "__dict__"), T
    assert (st.pair.off1, st.pair.offr, st.pair.offk) == tuple(st.pair.t.offs) and st.pair.rvv is None and st.pair.t.tabs is None
    t = st.pair.t  # (the pair tables read by name as well as by position, and a dict of the fields makes the record)
    assert t["ta"] is t.ta is t[0] and t["offs"] is t.offs and E._rec(E.PairTables, t._asdict()) == t


@pytest.mark.parametrize("B", [2, 600])
@pytest.mark.parametrize("prec", ["fp16", "split", "fp32"])
@pytest.mark.parametrize("net", ["pos", "feat"])
def test_plan_tables_name_the_launches_they_mean(nets, monkeypatch, net, prec, B):
    hp, sd = nets[net]
    for knobs in KNOBS:
        with monkeypatch.context() as mp:
            for k in {k for ks in KNOBS for k in ks}:
                mp.delenv(k, raising=False)
            for k, v in knobs.items():
                mp.setenv(k, v)
            e = E.DenoiserEngine(hp, sd, B, torch.device("cpu"), prec=prec)
        ops, n = e.ops, len(e.ops)
        assert [x.op for x in e.plan] == ops, knobs
        assert ops[e._prep_idx].kind == E.OP_PREP_POINTS, knobs
        assert e.eps_copy_idx == n - 1 and ops[e.eps_copy_idx].kind == E.OP_COPY_COLS, knobs
        assert all(ops[k].kind == E.OP_COPY_COLS for k in e.xyz_copy_idx), knobs
        if e.head is not None:
            assert len(e.head["idx"]) == 2 and all(ops[k].kind == E.OP_GEMM and ops[k].i[0] == 16 * B for k in e.head["idx"]), knobs
        if e.point_chain is not None:
            assert len(e.point_chain["idx"]) == 4 and all(ops[k].kind == E.OP_GEMM for k in e.point_chain["idx"]), knobs
        for d in (e.gemm_flops, e.gemm_bytes, e.kernel_names):
            assert all(0 <= k < n for k in d), knobs
        for part, kind in NAMED:
            named = {k for k, v in e.kernel_names.items() if part in v}
            assert all(ops[k].kind == kind for k in named), (knobs, part)
            if kind != E.OP_ATTN_TAIL:  # (the fp16 attention tail has no recorded name)
                assert named == {k for k, o in enumerate(ops) if o.kind == kind}, (knobs, part)
