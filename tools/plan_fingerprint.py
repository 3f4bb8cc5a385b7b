"""Canonical text form of the denoiser plans and the samplers' step plans, for comparing two trees of this repository:

    python tools/plan_fingerprint.py --root <tree A> > a.txt;  python tools/plan_fingerprint.py --root <tree B> > b.txt;  cmp a.txt b.txt

Plans are built on the CPU device (no GPU, no library: `lib()` is stubbed; `torch.cuda.Stream` is stubbed so that the samplers
construct).  Every pointer is written as (ordinal of the arena tensor by first appearance in the walk, byte offset) with bit 0 kept
as a flag; host blocks an op points to (op pairs, chain tables, pp-stage records, argument blocks) are expanded in place.  For batch 2
each tensor's bytes are hashed, descriptor blobs (uint8) with the pointers inside them made canonical the same way.
Only attributes every tree has had are read: ops, the accounting dicts, the index tables, flops, step_ops, the keep-alive lists."""
import argparse
import bisect
import ctypes
import hashlib
import os
import sys

KNOBS = [{}, {"SLIDE_GEMM_CHAIN": "256"}, {"SLIDE_GEMM_CHAIN": "100000"}, {"SLIDE_GX_DUAL": "0"}, {"SLIDE_CHAIN_P": "0"}, {"SLIDE_PP": "1"},
         {"SLIDE_FOLD_COPIES": "0"}, {"SLIDE_SA_CHAIN": "0"}, {"SLIDE_GXS_CHAIN": "0", "SLIDE_GX_DUAL": "0"}, {"SLIDE_MERGE_Q": "0"},
         {"SLIDE_POINT_CHAIN": "0"}, {"SLIDE_TWO_LANES": "1"}]
FORM_BATCHES = (1, 256, 257, 512, 513, 1024, 1025, 1364, 1365, 2048, 2049)  # test_batch_size_plan_forms


class Walk:
    """pointer -> canonical form, over one engine's arena and host blocks"""

    def __init__(self, engine, samplers, hashed):
        import numpy as np
        import torch
        self.np, self.torch, self.hashed = np, torch, hashed
        tensors = []

        def collect(x):
            if torch.is_tensor(x):
                if x.numel():
                    tensors.append(x)
            elif isinstance(x, (tuple, list)):
                for y in x:
                    collect(y)
        collect(engine.A.keep)
        tensors.sort(key=lambda t: t.data_ptr())
        self.tensors, self.starts = tensors, [t.data_ptr() for t in tensors]
        self.ordinal, self.order = {}, []
        self.host = {}  # address -> ("name", object)
        for name in ("_dual_keep", "_chain_p_keep", "_chain_keep", "_pp_keep"):
            for blk in getattr(engine, name, None) or []:
                self.host[blk.ctypes.data if isinstance(blk, np.ndarray) else ctypes.addressof(blk)] = blk
        for owner in [engine] + list(samplers):
            for name in ("_fwd_chain_args", "_chain_args", "_head_args"):
                blk = getattr(owner, name, None)
                if blk is not None:
                    self.host[ctypes.addressof(blk)] = blk
        for x in engine.A.keep:  # (SLIDE_OP_BLOCK_BODY argument blocks)
            if isinstance(x, tuple) and isinstance(x[0], ctypes.Structure):
                self.host[ctypes.addressof(x[0])] = x[0]

    def tensor_at(self, addr):
        k = bisect.bisect_right(self.starts, addr) - 1
        if k >= 0:
            t = self.tensors[k]
            if addr < t.data_ptr() + t.numel() * t.element_size():
                return t
        return None

    def ptr(self, v):
        if not v:
            return "null"
        flag, addr = v & 1, v & ~1
        if v in self.host or addr in self.host:
            return "host%s" % self.value(self.host.get(v, self.host.get(addr)))
        t = self.tensor_at(addr)
        if t is None:
            raise SystemExit("pointer %#x is neither in the arena nor a known host block" % v)
        key = t.data_ptr()
        if key not in self.ordinal:
            self.ordinal[key] = len(self.order)
            self.order.append(t)
        return "(T%d+%d%s)" % (self.ordinal[key], addr - key, " flag" if flag else "")

    def value(self, x):
        np = self.np
        if isinstance(x, ctypes.Structure):
            return "%s{%s}" % (type(x).__name__, ", ".join("%s=%s" % (n, self.field(getattr(x, n), ct)) for n, ct in x._fields_))
        if isinstance(x, ctypes.Array):
            return "[%s]" % ", ".join(self.field(y, x._type_) for y in x)
        if isinstance(x, np.ndarray):  # pp-stage record: [n, B] + 16 words per step (kind, then pointers and sizes; see _merge_pp)
            n, out = int(x[0]), [int(x[0]), int(x[1])]
            for s in range(n):
                w = [int(v) for v in x[2 + 16 * s:18 + 16 * s]]
                npt = 6 if w[0] == 0 else 14
                out.append("step[%d, %s, %s]" % (w[0], ", ".join(self.ptr(v) for v in w[1:npt]), ", ".join(str(v) for v in w[npt:])))
            return "pp[%s]" % ", ".join(str(v) for v in out)
        raise TypeError(type(x))

    def field(self, v, ct):
        if ct is ctypes.c_void_p:
            return self.ptr(v)
        if isinstance(v, (ctypes.Structure, ctypes.Array)):
            return self.value(v)
        return repr(float(v)) if ct is ctypes.c_float else str(int(v))

    def tensor_table(self):
        """one line per tensor the walk met (the list grows while descriptor blobs name further tensors)"""
        lines, k = [], 0
        while k < len(self.order):
            t = self.order[k]
            line = "T%d %s %s" % (k, tuple(t.shape), str(t.dtype).replace("torch.", ""))
            if self.hashed:
                raw = t.contiguous().view(-1).view(self.torch.uint8).numpy().copy()
                if t.dtype == self.torch.uint8 and raw.size % 8 == 0:  # descriptor blob: pointers inside it
                    words = raw.view(self.np.uint64)
                    names = []
                    for q, w in enumerate(words):
                        w = int(w)
                        if w > 0xFFFFFFFF and self.tensor_at(w & ~1) is not None:
                            names.append("%d:%s" % (q, self.ptr(w)))
                            words[q] = 0
                    line += " ptrs[%s]" % " ".join(names)
                line += " " + hashlib.sha1(raw.tobytes()).hexdigest()[:16]
            lines.append(line)
            k += 1
        return lines


def describe(out, tag, engine, samplers, hashed, names):
    w = Walk(engine, samplers, hashed)
    out.append("== %s" % tag)

    def ops_block(label, ops):
        out.append("%s: %d ops" % (label, len(ops)))
        for k, o in enumerate(ops):
            out.append("  %d %s i=%s f=%s p=[%s]" % (k, names.get(o.kind, o.kind), list(o.i), [repr(float(v)) for v in o.f],
                                                      ", ".join(w.ptr(v) for v in o.p)))

    def tables(label, obj):
        for k_ in ("gemm_flops", "gemm_bytes", "kernel_names"):
            d = getattr(obj, k_)
            out.append("%s.%s: %s" % (label, k_, ", ".join("%d=%s" % (k, d[k]) for k in sorted(d))))
    ops_block("ops", engine.ops)
    tables("engine", engine)
    head, pc = getattr(engine, "head", None), getattr(engine, "point_chain", None)
    out.append("xyz_copy_idx=%s eps_copy_idx=%s _prep_idx=%s head.idx=%s point_chain.idx=%s flops=%d" % (
        list(engine.xyz_copy_idx), engine.eps_copy_idx, engine._prep_idx, None if head is None else list(head["idx"]),
        None if pc is None else list(pc["idx"]), engine.flops))
    ops_block("step_ops", list(engine.step_ops))
    for label, smp in zip(("sampler", "sampler2"), samplers):
        ops_block(label + ".step_ops", list(smp.step_ops))
        ops_block(label + ".begin_ops", list(smp.begin_ops) if smp.begin_ops is not None else [])
        tables(label, smp)
    out.extend(w.tensor_table())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="tree to import slide_amd from")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-samplers", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    from slide_amd import configs, diffusion, engine as E, model_spec
    from slide_amd.synth import synth_state_dict
    assert os.path.abspath(E.__file__).startswith(os.path.abspath(args.root)), E.__file__
    E.lib = lambda: None  # (a plan is built without the library; it cannot run)

    class _NoStream:
        cuda_stream = 0

        def __init__(self, *a, **k):
            pass
    torch.cuda.Stream = _NoStream
    names = {v: k for k, v in vars(E).items() if k.startswith("OP_") and isinstance(v, int)}
    dev = torch.device("cpu")
    nets = {}
    for net, cfg in (("pos", configs.position_ddpm_config()), ("feat", configs.feature_ddpm_config())):
        hp = cfg["pointnet_config"]
        nets[net] = (hp, synth_state_dict(model_spec.denoiser_param_spec(hp)), cfg)
    knob_names = sorted({k for ks in KNOBS for k in ks})
    out = []

    def case(net, prec, B, knobs, samplers=True):
        for k in knob_names:
            os.environ.pop(k, None)
        os.environ.update(knobs)
        hp, sd, cfg = nets[net]
        tag = "%s %s B=%d %s" % (net, prec, B, " ".join("%s=%s" % kv for kv in sorted(knobs.items())) or "default")
        describe(out, tag + " forward", E.DenoiserEngine(hp, sd, B, dev, prec=prec), [], B == 2, names)
        if samplers and not args.no_samplers:
            if net == "pos":
                dc = dict(cfg["diffusion_config"], T=10)
                smp = diffusion.PositionSampler(hp, sd, B, dev, dc, prec=prec, seed=5)
            else:
                dc = dict(cfg["standard_diffusion_config"], num_diffusion_timesteps=10)
                smp = diffusion.FeatureSampler(hp, sd, B, dev, dc, prec=prec, seed=5)
            describe(out, tag + " sampler", smp.engine, [smp], B == 2, names)
        print(tag, file=sys.stderr)
    for net in ("pos", "feat"):
        for prec in ("fp16", "split", "fp32"):
            for B in (2, 600):
                for knobs in KNOBS:
                    case(net, prec, B, knobs)
    for B in FORM_BATCHES:
        case("feat", "fp16", B, {}, samplers=False)
    text = "\n".join(out) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    print("sha256 %s  (%d lines)" % (hashlib.sha256(text.encode()).hexdigest(), len(out)), file=sys.stderr)


if __name__ == "__main__":
    main()
