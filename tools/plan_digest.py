#!/usr/bin/env python
"""Digest of a built DenoiserEngine plan that depends neither on addresses nor on the order of arena allocations: two checkouts
build the same plan exactly when their digests are equal (a plan builds on torch.device("cpu"), and a plan is nothing but bytes).

  python tools/plan_digest.py [--root CHECKOUT] [--jobs N] --out FILE        digests of the whole matrix, one line per plan
  python tools/plan_digest.py --compare PARENT_FILE BRANCH_FILE [--md FILE]  the two columns side by side; exit 1 unless all equal

What goes in: every entry of `plan` (kind, i, f, p, flops, nbytes, name, sorted roles), `step_ops`, `cond_op`, `table_ops`, the
results of `plan_tables`, the `head` / `point_chain` records and `flops`.  Every pointer is replaced by (canonical id of the block
that owns it, byte offset); ids are given in order of first reference.  A block is an arena tensor or a host block (the merge passes'
keep lists, the forward point chain's arguments, a launch's BodyArgs).  A block's content enters as dtype, shape and SHA-256; in
host blocks and uint8 descriptor blobs the pointers are first replaced by their canonical reference, recursively: a ctypes block by
its pointer fields, a blob by every aligned 64-bit word that falls inside a known block.  A pointer that resolves to no block is
counted; the count must be 0."""
import argparse
import bisect
import ctypes
import functools
import hashlib
import json
import os
import sys

KNOBS = ["", "SLIDE_GX=0", "SLIDE_GXS=0", "SLIDE_CM=0", "SLIDE_GLDS=0", "SLIDE_PAIR_FUSED=0", "SLIDE_PAIR_NORM_V2=1",
         "SLIDE_GX=0 SLIDE_SPLIT_FIRST=32", "SLIDE_ATTN_TAIL=0", "SLIDE_TAIL_SPLIT=0", "SLIDE_FUSE_FIN=0", "SLIDE_PACKED_VECS=0",
         "SLIDE_GX_N64=0", "SLIDE_GX_N64W=0", "SLIDE_BODY=1", "SLIDE_CM_TABLES=1", "SLIDE_GX=0 SLIDE_GATHER=0", "SLIDE_GX=0 SLIDE_XS=auto",
         "SLIDE_FM=0", "SLIDE_GEMM_CHAIN=256", "SLIDE_GX_DUAL=0", "SLIDE_CHAIN_P=0", "SLIDE_PP=1", "SLIDE_FOLD_COPIES=0", "SLIDE_SA_CHAIN=0",
         "SLIDE_GXS_CHAIN=0", "SLIDE_MERGE_Q=0", "SLIDE_POINT_CHAIN=0", "SLIDE_TWO_LANES=1", "SLIDE_PERSISTENT=1",
         "SLIDE_POINT_CHAIN_WIDE=0", "SLIDE_GLDS_WIDE=1 SLIDE_GATHER=0", "SLIDE_CBW4_TILES=1", "SLIDE_CBW1_TILES=8", "SLIDE_TAIL_OCC3=1",
         "SLIDE_TAIL_WIDE=4", "SLIDE_TAIL_WIDE=1000", "SLIDE_TAIL8=1", "SLIDE_TAIL_RX=0", "SLIDE_STAGGER_US=0.07", "SLIDE_BODY=2",
         "SLIDE_GX=0 SLIDE_XS=auto SLIDE_XS_CBW=4", "SLIDE_GX=0 SLIDE_XS=auto SLIDE_XS_OCC=2", "SLIDE_PERSISTENT=2",
         "SLIDE_POINT_CHAIN_PACKED=0"]


def matrix():
    """the plans of the acceptance matrix: (net, prec, batch, per_sample_t, t_table, knobs)"""
    forms = [(2, True, 0, k) for k in KNOBS] + [(600, True, 0, ""), (2, False, 8, ""), (600, False, 8, "")]
    return [(net, prec) + f for net in ("pos", "feat") for prec in ("fp16", "split", "fp32") for f in forms]


def case_name(case):
    net, prec, B, per_sample_t, t_table, knobs = case
    return "%s %s B=%d %s{%s}" % (net, prec, B, "" if per_sample_t else "t_table=%d " % t_table, knobs)


@functools.lru_cache(maxsize=None)
def _zero_sha(nbytes):
    h, chunk = hashlib.sha256(), bytes(1 << 20)
    for _ in range(nbytes >> 20):
        h.update(chunk)
    h.update(bytes(nbytes & ((1 << 20) - 1)))
    return h.hexdigest()


def _sha(a):
    """SHA-256 of a contiguous uint8 array (all-zero buffers, the activations, through the cache above)"""
    return hashlib.sha256(a).hexdigest() if a.any() else _zero_sha(a.size)


class _Digest:
    def __init__(self, engine):
        import numpy as np
        import torch
        self.np, self.torch = np, torch
        blocks = [t for t in engine.A.keep if torch.is_tensor(t)]  # (_emit_block_body appends a non-tensor entry)
        for k in ("_chain_keep", "_dual_keep", "_chain_p_keep", "_pp_keep"):
            blocks += getattr(engine, k, [])
        blocks += [b for b in [getattr(engine, "_fwd_chain_args", None)] + [e.body for e in engine.plan] if b is not None]
        spans = sorted(((self._span(b), b) for b in blocks), key=lambda s: s[0])
        self.starts, self.spans = [s[0][0] for s in spans], spans
        self.ids, self.content, self.unresolved = {}, [], 0

    def _span(self, b):
        if self.torch.is_tensor(b):
            return b.data_ptr(), max(b.numel() * b.element_size(), 1)
        if isinstance(b, self.np.ndarray):
            return b.ctypes.data, b.nbytes
        return ctypes.addressof(b), ctypes.sizeof(b)

    def _find(self, p):
        k = bisect.bisect_right(self.starts, p) - 1
        if k >= 0 and p < self.spans[k][0][0] + self.spans[k][0][1]:
            return self.spans[k]
        return None

    def ref(self, p, scan=False):
        """canonical form of a pointer; scan: p is a word of a blob that may be no pointer at all (then None)"""
        if not p:
            return 0
        hit = self._find(p)
        if hit is None:
            if scan:
                return None
            self.unresolved += 1
            return "unresolved"
        (start, _), b = hit
        if start not in self.ids:
            self.ids[start] = len(self.ids)
            self.content.append(None)
            self.content[self.ids[start]] = self._content(b)
        return [self.ids[start], p - start]

    def _words(self, raw):
        """(refs, sha) of a blob: its aligned 64-bit words that point into a block, and its bytes without them"""
        raw = self.np.frombuffer(bytearray(raw), dtype=self.np.uint8)
        w = raw[:raw.size // 8 * 8].view(self.np.uint64)
        lo, hi = self.starts[0], self.spans[-1][0][0] + self.spans[-1][0][1]
        refs = []
        for k in self.np.nonzero((w >= lo) & (w < hi))[0]:
            r = self.ref(int(w[k]), scan=True)
            if r is not None:
                refs.append([int(k), r])
                w[k] = 0
        return refs, _sha(raw)

    def _struct(self, s):
        """a ctypes structure or array by its fields: pointer fields as references"""
        if isinstance(s, ctypes.Array):
            if s._type_ is ctypes.c_void_p:
                return [self.ref(v) for v in s]
            return [self._struct(v) if isinstance(v, (ctypes.Structure, ctypes.Array)) else self._scalar(v) for v in s]
        out = []
        for name, tp in s._fields_:
            v = getattr(s, name)
            if tp is ctypes.c_void_p:
                out.append(self.ref(v))
            elif isinstance(v, (ctypes.Structure, ctypes.Array)):
                out.append(self._struct(v))
            else:
                out.append(self._scalar(v))
        return out

    @staticmethod
    def _scalar(v):
        return v.hex() if isinstance(v, float) else v

    def _content(self, b):
        if self.torch.is_tensor(b):
            a = b.detach().contiguous().view(-1).view(self.torch.uint8).numpy()
            head = [str(b.dtype), list(b.shape)]
            return head + (list(self._words(a.tobytes())) if b.dtype == self.torch.uint8 else [_sha(a)])
        if isinstance(b, self.np.ndarray):
            return [str(b.dtype), list(b.shape)] + list(self._words(b.tobytes()))
        return [type(b).__name__, self._struct(b)]

    def op(self, o):
        return None if o is None else [o.kind, list(o.i), [v.hex() for v in o.f], [self.ref(p) for p in o.p]]


def plan_record(engine):
    """(the address-free record of a built plan, number of unresolved pointers)"""
    from slide_amd import engine as E
    d = _Digest(engine)
    rec = {"plan": [[d.op(e.op), e.flops, e.nbytes, e.name, sorted(e.roles)] for e in engine.plan]}
    for k in ("step_ops", "cond_op", "table_ops"):
        v = getattr(engine, k, None)
        rec[k] = None if v is None else d.op(v) if isinstance(v, E.SlideOp) else [d.op(o) for o in v]
    rec["tables"] = {k: v for k, v in E.plan_tables(engine.plan).items() if k != "ops"}
    for k in ("head", "point_chain"):
        v = getattr(engine, k, None)
        rec[k] = None if v is None else {n: d.ref(x.data_ptr()) if d.torch.is_tensor(x) else x for n, x in sorted(v.items())}
    rec["flops"] = engine.flops
    rec["blocks"] = d.content
    return rec, d.unresolved


def plan_digest(engine):
    """(hex digest of a built plan, number of unresolved pointers)"""
    rec, unresolved = plan_record(engine)
    return hashlib.sha256(json.dumps(rec, sort_keys=True, default=int).encode()).hexdigest(), unresolved


def set_knobs(knobs):
    """the environment with exactly these SLIDE_* plan knobs ("A=1 B=2")"""
    for k in [k for k in os.environ if k.startswith("SLIDE_") and k not in ("SLIDE_HIP_LIB", "SLIDE_EXPERIMENTS")]:
        del os.environ[k]
    os.environ.update(kv.split("=") for kv in knobs.split())


@functools.lru_cache(maxsize=None)
def _net(net):
    from slide_amd import configs, model_spec
    from slide_amd.synth import synth_state_dict
    hp = (configs.position_ddpm_config() if net == "pos" else configs.feature_ddpm_config())["pointnet_config"]
    return hp, synth_state_dict(model_spec.denoiser_param_spec(hp))


def run_case(case):
    import torch
    from slide_amd import engine as E
    net, prec, B, per_sample_t, t_table, knobs = case
    set_knobs(knobs)
    try:
        hp, sd = _net(net)
        e = E.DenoiserEngine(hp, sd, B, torch.device("cpu"), prec=prec, per_sample_t=per_sample_t, t_table=t_table)
        return (case_name(case),) + plan_digest(e)
    except Exception as exc:  # a plan that does not build is a result too: both checkouts must fail alike
        return case_name(case), "build error: %s: %s" % (type(exc).__name__, exc), 0


def _use_root(root):
    sys.path.insert(0, os.path.abspath(root))


def compare(parent, branch, md):
    rows = [[ln.rstrip("\n").split("\t") for ln in open(f)] for f in (parent, branch)]
    a, b = ({r[0]: r[1:] for r in rs} for rs in rows)
    names = [r[0] for r in rows[0]] + [n for n in b if n not in a]
    bad = [n for n in names if a.get(n) != b.get(n)]
    unresolved = sum(int(v[1]) for t in (a, b) for v in t.values())
    lines = ["| plan | parent | branch | |", "|---|---|---|---|"]
    lines += ["| %s | %s | %s | %s |" % (n, a.get(n, ["-"])[0][:16], b.get(n, ["-"])[0][:16], "DIFFERS" if n in bad else "=") for n in names]
    lines += ["", "%d plans, %d differ, %d distinct digests, %d unresolved pointers" %
              (len(names), len(bad), len({v[0] for v in a.values()}), unresolved)]
    if md:
        open(md, "w").write("\n".join(lines) + "\n")
    print(lines[-1])
    return 1 if bad or unresolved else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."), help="checkout to import slide_amd from")
    ap.add_argument("--jobs", type=int, default=1)
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("PARENT", "BRANCH"))
    ap.add_argument("--md", help="with --compare: write the table here")
    a = ap.parse_args()
    if a.compare:
        return compare(a.compare[0], a.compare[1], a.md)
    cases = matrix()
    if a.jobs > 1:
        import multiprocessing as mp
        with mp.get_context("spawn").Pool(a.jobs, initializer=_use_root, initargs=(a.root,)) as pool:
            res = pool.map(run_case, cases, chunksize=1)
    else:
        _use_root(a.root)
        res = [run_case(c) for c in cases]
    text = "".join("%s\t%s\t%d\n" % r for r in res)
    if a.out:
        open(a.out, "w").write(text)
    else:
        sys.stdout.write(text)
    n_err = sum(r[1].startswith("build error") for r in res)
    print("%d plans, %d build errors, %d unresolved pointers, %d distinct digests" %
          (len(res), n_err, sum(r[2] for r in res), len({r[1] for r in res})), file=sys.stderr)
    return 1 if n_err or any(r[2] for r in res) else 0


if __name__ == "__main__":
    sys.exit(main())
