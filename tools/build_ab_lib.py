#!/usr/bin/env python
"""Build a second kernel library for same-box A/B: the in-tree sources, except the listed kernel files taken
from git revision REV, linked into tools/ab_so/_hq_kernels<ext> (load it with HQ_KERNELS_DIR=tools/ab_so;
AB_DIR=tools/<name> picks another directory; HQ_KERNEL_CFLAGS="-DHQ_EPI_DIAG=1 ..." adds lab defines to THIS build
only — the production build never reads it).

    python tools/build_ab_lib.py HEAD ml_recipe_distributed_pytorch_amd/csrc/kernels/gemm_nt_v3.hip

A file is overlaid whole, so REV must define the same functions in it as the tree does: across the commit that split
norm.hip (into norm / embed / sort / rowops.hip, the span head into heads.hip) and moved the fp8 quantisers and amax
folds from gemm_fp8.hip to fp8.hip, name every file the subject moved between (and include/hq_kernels.h), or the
link has duplicate or missing hq_* symbols; a subject whose file does not exist at REV (embed / sort / rowops.hip)
cannot be overlaid from before that commit — build that revision whole in a worktree instead.  Likewise across the
commit that split the fp32 ops file into f32_embed / f32_norm / f32_rowops / f32_attention.hip: from before it, build the whole revision in a worktree
(AB_DIR still picks where the library goes).  And across the commit that split attention.hip into attention_fwd.hip,
attention_bwd.hip and include/hq_attn.h: from before it, build the parent whole in a worktree.  The same holds across
the commit that split gemm.hip into gemm_nt.hip, gemm_nt_v1 / _vs / _v2 / _v3.hip and include/hq_gemm_tile.h, hq_gemm_nt.h.
"""
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    rev, files = sys.argv[1], sys.argv[2:]
    from ml_recipe_distributed_pytorch_amd.csrc import build as b
    out_dir = os.path.join(ROOT, os.environ.get("AB_DIR", os.path.join("tools", "ab_so")))
    tmp = os.path.join(out_dir, "src")
    if os.path.exists(tmp):
        shutil.rmtree(tmp)
    shutil.copytree(b.HERE, tmp, ignore=shutil.ignore_patterns("build"))
    for f in files:
        rel = os.path.relpath(os.path.join(ROOT, f), b.HERE)
        with open(os.path.join(tmp, rel), "wb") as fh:
            fh.write(subprocess.check_output(["git", "show", f"{rev}:{f}"], cwd=ROOT))
    here, pkg = b.HERE, b.PKG
    try:
        b.HERE, b.PKG = tmp, out_dir
        lab = [f for f in os.environ.get("HQ_KERNEL_CFLAGS", "").split() if f.startswith("-D")]
        out = b.build_kernels(8, lab_defines=lab)
    finally:
        b.HERE, b.PKG = here, pkg
    print(out)


if __name__ == "__main__":
    main()
