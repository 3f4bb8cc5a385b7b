"""Every SLIDE_* environment variable of the package, declared once: name, kind, default, scope and what it switches.

  python -m slide_amd.knobs        the table with the current values

Kinds (a default is the string an unset variable stands for; None: no string at all):
  flag   off exactly when the string is "0" (so "" and "00" are on)
  int    int(string)
  float  float(string)
  text   the string itself: the code compares it
  opt    the string itself, None when the variable is unset

Scopes:
  plan     steers how DenoiserEngine and the samplers build a plan; resolved once per engine (`snapshot`, engine.knobs)
  live     read from the environment where it is used, every time (`read`): the module path, the generation CLIs, the loader
  library  read by libslide_hip.so itself (getenv, once per process); Python parses only the two the plan builder has to mirror

`read` and `snapshot` parse the environment as it is when they are called: nothing here remembers a value.  bench.py's own
switches (SLIDE_BENCH_*, SLIDE_REPLAY, ...) are bench.py's and are not listed."""
import os
from typing import NamedTuple, Optional


class Knob(NamedTuple):
    name: str
    kind: str
    default: Optional[str]
    scope: str
    doc: str


_PARSE = {"flag": lambda s: s != "0", "int": int, "float": float, "text": lambda s: s, "opt": lambda s: s}


def _table(scope, rows):
    return [Knob(n, k, d, scope, doc) for n, k, d, doc in rows]


TABLE = _table("plan", [
    # engine.py
    ("SLIDE_GLDS", "flag", "1", "fp16 plans use the LDS-DMA ring kernels (0: the register-staged kernel for every GEMM)"),
    ("SLIDE_GLDS_WIDE", "int", "0", "1: 64-deep K chunks (row-major operands), 2: eight-wave 256x256 tiles, 3: no split-K small-launch "
                                    "kernel, 4: eight-wave narrow tiles"),
    ("SLIDE_CM", "flag", "1", "chunk-major activations and weights for the 128- / 256-row ring kernels (0: row-major everywhere)"),
    ("SLIDE_CM_TABLES", "flag", "0", "chunk-major second copies of the gathered per-point tables as well"),
    ("SLIDE_GX", "flag", "1", "pair decomposition of the blocks' first layers + generated-X GEMMs (0: first layers over gathered inputs)"),
    ("SLIDE_GXS", "flag", "1", "split plans: the pair decomposition in the split arithmetic (0: the fp32-structured plan)"),
    ("SLIDE_XS", "text", "", "X-stationary GEMM kernel: \"\" off, \"auto\", or the row-tile log2 sizes \"7,8\"; any value turns "
                             "chunk-major storage off"),
    ("SLIDE_XS_CBW", "text", "2", "X-stationary kernel: \"4\" = four-block column tiles"),
    ("SLIDE_XS_OCC", "opt", None, "X-stationary kernel: cap on its workgroups per CU (empty: no cap)"),
    ("SLIDE_TWO_LANES", "flag", "0", "score / value branches of an attention block on two streams"),
    ("SLIDE_FM", "flag", "1", "u / mo of the register-X attention tails stored fragment-major (0: chunk-major)"),
    ("SLIDE_ATTN_TAIL", "flag", "1", "scores + values + soft-max + sum in the fused attention tail (0: two GEMMs + combine launch)"),
    ("SLIDE_TAIL_SPLIT", "flag", "1", "split plans: the same tail in the split arithmetic (0: two GEMMs + combine launch)"),
    ("SLIDE_TAIL_OCC3", "flag", "0", "attention tail: two-stage ring at three workgroups per CU"),
    ("SLIDE_TAIL_WIDE", "opt", None, "attention tail: four-wave 256x128 form for layers of at least this many channel blocks; set at "
                                     "all, it turns fragment-major storage off"),
    ("SLIDE_BODY", "text", "0", "\"0\": three launches per block; otherwise the one-launch block body for FP0-sized blocks, \"2\": "
                                "for SA0 too"),
    ("SLIDE_PACKED_VECS", "flag", "1", "descriptor buffers carry [bias | gamma | beta] behind the descriptors, pointer bit 0 says so "
                                       "(0: plain pointer); the module path reads it too, per call"),
    ("SLIDE_CBW4_TILES", "int", "1000", "minimum tile count for 128-channel tiles"),
    ("SLIDE_CBW1_TILES", "int", "0", "maximum tile count for 32-channel tiles"),
    ("SLIDE_STAGGER_US", "float", "0", "start stagger of the odd wave slot; A/B switches ride on the same field"),
    ("SLIDE_PERSISTENT", "int", "0", "1: tile counter per XCD, 2: static tile lists"),
    ("SLIDE_GX_N64", "text", "1", "generated-X GEMMs on 64-channel tiles (\"0\": 128-channel tiles)"),
    ("SLIDE_GX_N64W", "flag", "1", "64-channel tiles at two workgroups per CU where the 128-channel grid would leave CUs empty"),
    ("SLIDE_GX_DUAL", "flag", "1", "the mode-1 and mode-0 generated-X GEMMs of an FP block in one launch (0: two launches)"),
    ("SLIDE_GXS_CHAIN", "flag", "1", "split plans: second_mlp -> rest_mlp of an SA block in one launch"),
    ("SLIDE_SA_CHAIN", "flag", "1", "SA second_mlp -> rest_mlp in one launch with h2 in registers"),
    ("SLIDE_CHAIN_P", "flag", "1", "SA blocks: query GEMM + Mlp chain in one launch (0: apart)"),
    ("SLIDE_PAIR_FUSED", "flag", "1", "per-point GEMM + pair-table pass in one launch (0: GEMM -> fp32 y -> pair-norm launch)"),
    ("SLIDE_PAIR_NORM_V2", "flag", "0", "one 1024-thread workgroup per sample finalises the joint GroupNorm too"),
    ("SLIDE_SPLIT_FIRST", "int", "1000000", "minimum feature width for evaluating a block's first layer per point"),
    ("SLIDE_FUSE_FIN", "flag", "1", "GroupNorm finalisation of the score branch folded into the per-point query GEMM"),
    ("SLIDE_GATHER", "flag", "1", "first GEMM of an SA / FP block DMA-gathers the neighbour rows (0: grouped input assembled in memory)"),
    ("SLIDE_MERGE_Q", "flag", "1", "attention queries ride on a shared per-point GEMM (0: one query GEMM per attention block)"),
    ("SLIDE_FOLD_COPIES", "flag", "1", "COPY launches folded into the producers of their sources (0: separate launches)"),
    ("SLIDE_GEMM_CHAIN", "int", "0", "largest chain (KB of weights) of consecutive per-point GEMMs merged into one launch"),
    ("SLIDE_PP", "flag", "0", "split plans: runs of 16-row launches as one per-point stage launch"),
    ("SLIDE_POINT_CHAIN", "flag", "1", "FP0's second Mlp + the output head offered to the samplers as one launch (0: four launches)"),
    ("SLIDE_POINT_CHAIN_WIDE", "flag", "1", "the point chain in the split arithmetic (0: fp16 operands)"),
    ("SLIDE_POINT_CHAIN_PACKED", "flag", "1", "the point chain reads its weights as one buffer of packed MFMA fragments (0: row-major)"),
    # diffusion.py
    ("SLIDE_FUSE_PREP", "flag", "1", "feature sampler: point preparation once per chain (0: one launch per step)"),
    ("SLIDE_HEAD_UPDATE", "flag", "0", "output head + DDPM update in one launch"),
    ("SLIDE_POINT_CHAIN_UPDATE", "flag", "0", "the feature DDPM's update rides on the point-chain launch too"),
    ("SLIDE_ABL_DROP", "opt", None, "TIMING ablation: launches whose kernel name contains one of these substrings are left out"),
    ("SLIDE_STREAM_PRIO", "opt", None, "\"<position>,<feature>\" HIP stream priorities of the chains (-1 high)"),
    ("SLIDE_POS_CUS", "opt", None, "compute units the position chains' streams may use (0 = all)"),
    ("SLIDE_FEAT_CUS", "opt", None, "compute units the feature chains' streams may use (0 = all)"),
    ("SLIDE_CU_MASK_FROM", "int", "0", "first compute unit of those masks"),
]) + _table("live", [
    ("SLIDE_MODULE_PREC", "text", "fp32", "module path: \"fp16\" = fp16 MFMA operands, fp32 accumulate"),
    ("SLIDE_MODULE_STATS", "flag", "1", "module path: GroupNorm statistics from the producing GEMM's epilogue"),
    ("SLIDE_MODULE_DEFER", "flag", "1", "module path: deferred normalisation (fp16 operands only)"),
    ("SLIDE_MODULE_PAIR", "flag", "1", "fp16 module path: convolutions over grouped inputs by the pair decomposition"),
    ("SLIDE_MODULE_FUSE_ATTEND", "flag", "1", "fp16 module path: score GEMM + soft-max + weighted sum in one launch"),
    ("SLIDE_MODULE_SPLIT_QK", "flag", "1", "fp16 module path: AttentionModule without the [q | k] concatenation"),
    ("SLIDE_MODULE_CBW4", "flag", "0", "module path: 128-channel tiles"),
    ("SLIDE_PINNED_TABLES", "flag", "1", "module path: descriptor tables through pinned slots + asynchronous copies"),
    ("SLIDE_POS_MULT", "int", "2", "generation: the position chain runs over this multiple of the batch"),
    ("SLIDE_SHARE_GPU", "flag", "0", "generation CLIs: all ranks on device 0 over gloo"),
    ("SLIDE_HIP_LIB", "opt", None, "path of an alternative libslide_hip.so (read by _lib.py at import)"),
    ("SLIDE_EXPERIMENTS", "text", "0", "anything but \"\" and \"0\": load the experiments library (read by _lib.py at import)"),
    ("SLIDE_ALLOW_SPILLS", "flag", "0", "a spilling kernel in the product build is a warning, not an error (read by build.py)"),
]) + _table("library", [
    ("SLIDE_TAIL_RX", "flag", "1", "fp16 attention tails load their X fragments straight into registers (0: the LDS-ring form)"),
    ("SLIDE_TAIL8", "flag", "0", "eight-wave 256x128 attention tail"),
    ("SLIDE_TAIL_ABL", "opt", None, "attention tail timing ablations (tools only)"),
    ("SLIDE_SA_SPLIT", "opt", None, "0: the SA chain never runs on two workgroups per sample"),
    ("SLIDE_SA_SPLIT_MAX", "opt", None, "launches of at most this many samples run the SA chain on two workgroups per sample"),
    ("SLIDE_XS_NSPLIT", "opt", None, "X-stationary kernel: cap on its column split"),
])
KNOBS = {k.name: k for k in TABLE}
assert len(KNOBS) == len(TABLE)


def read(name):
    """the current environment's value of one declared knob, parsed by its kind"""
    k = KNOBS[name]
    return _PARSE[k.kind](os.environ.get(name, k.default))


Snapshot = NamedTuple("Snapshot", [(k.name, object) for k in TABLE if k.scope != "live"])


def snapshot():
    """the plan-scope knobs, and the library-scope ones as Python mirrors them, as the environment has them now"""
    return Snapshot(*map(read, Snapshot._fields))


if __name__ == "__main__":
    for k in TABLE:
        print("%-26s %-8s default %-9s now %-9r %s" % (k.name, k.scope, k.default, read(k.name), k.doc))
