"""Instruction counts of the GroupNorm statistics passes of a kernel, from the compiler's assembly (no GPU needed).

    hipcc <the product flags of slide_amd/build.py> --cuda-device-only -S slide_amd/csrc/gemm_gx.hip -o gemm_gx.s
    python tools/ab/stats_isa_count.py gemm_gx.s 'sa_chain_kernelILi8E'

The kernel's text is cut at its workgroup barriers.  A statistics pass is a segment between two barriers that holds DPP adds: it
runs from the barrier that ends a K loop (the loop's last MFMA steps come first and are counted apart) to the first barrier of
group_stats.  Per segment: VALU instructions without the MFMAs, those with a DPP modifier, plain v_mov_b32, packed ops,
lane swaps, s_nop and scalar branches."""
import re
import sys


def kernel_text(lines, pattern):
    start = next(i for i, ln in enumerate(lines) if re.match(r"^_Z\w*:", ln) and pattern in ln.split(":")[0])
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[start + 1:end]


def count(seg):
    ops = [ln.split()[0] for ln in seg if ln.startswith("\t") and ln.strip() and not ln.startswith("\t.") and not ln.startswith("\t;")]
    valu = [o for o in ops if o.startswith("v_") and not o.startswith("v_mfma") and not o.startswith("v_accvgpr")]
    return {"valu": len(valu), "dpp": sum(o.endswith("_dpp") for o in valu), "v_mov_b32": sum(o.startswith("v_mov_b32_e32") for o in valu),
            "packed": sum(o.startswith("v_pk_") for o in valu), "cndmask": sum(o.startswith("v_cndmask") for o in valu),
            "swap": sum(o.startswith("v_permlane") for o in valu), "mfma": sum(o.startswith("v_mfma") for o in ops),
            "accvgpr": sum(o.startswith("v_accvgpr") for o in ops), "s_nop": sum(o == "s_nop" for o in ops),
            "branch": sum(o.startswith("s_cbranch") or o == "s_branch" for o in ops), "ds": sum(o.startswith("ds_") for o in ops)}


def main():
    lines = open(sys.argv[1]).read().split("\n")
    body = kernel_text(lines, sys.argv[2])
    segs, cur = [], []
    for ln in body:
        cur.append(ln)
        if ln.strip().startswith("s_barrier"):
            segs.append(cur)
            cur = []
    segs.append(cur)
    print("%d barriers" % (len(segs) - 1))
    for k, seg in enumerate(segs):
        c = count(seg)
        if c["dpp"] >= 8:
            print("segment %d (%d lines): %s" % (k, len(seg), " ".join("%s=%d" % kv for kv in c.items())))
            # its basic blocks (a label or a branch ends one): the groups-of-16 form and the other are alternatives of a pass,
            # a wave runs one of them
            blk, blocks = [], []
            for ln in seg:
                if re.match(r"^\.LBB\w+:", ln):
                    blocks.append(blk)
                    blk = []
                blk.append(ln)
                if ln.strip().startswith(("s_cbranch", "s_branch")):
                    blocks.append(blk)
                    blk = []
            blocks.append(blk)
            for b in blocks:
                cb = count(b)
                if cb["valu"] >= 16:
                    head = next((ln.split(":")[0] for ln in b if ln.startswith(".LBB")), "(fall-through)")
                    print("    block %-16s %s" % (head, " ".join("%s=%d" % kv for kv in cb.items() if kv[1])))


if __name__ == "__main__":
    main()
