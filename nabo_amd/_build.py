"""Builds libnabo_knn.so (HIP, gfx950) in-tree with hipcc.  No torch, no cmake.

    python -m nabo_amd._build [--force] [--verbose]
"""
import concurrent.futures
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
SO = os.path.join(HERE, "libnabo_knn.so")
SOURCES = ["api.hip", "plan.hip", "set_ref.hip", "bucket_order.hip", "query.hip", "pack.hip", "l2_topk.hip", "l2q_topk.hip", "l2c_topk.hip", "local_seeds.hip", "bucket_skip.hip", "refine.hip", "canberra.hip", "canberra_f32.hip", "canberra_bits.hip", "score_null.hip", "csr_build.hip", "comm.hip", "sharded.hip", "multi.hip", "host_graph.hip", "paths.hip", "classify.hip", "de_rank.hip", "pca_project.hip", "pca_fit.hip", "cell_qc.hip", "layout.hip", "umap.hip", "umap_transform.hip", "community.hip", "agglom.hip", "potential.hip", "bundle.hip", "render.hip", "mtx_ingest.hip", "counts.hip", "csv_ingest.hip"]
# per-file extra flags: -fno-honor-nans for the fp32 score kernel (scores are finite or +inf by construction; without it
# every fminf tree starts with two v_max canonicalisations, and on gfx950 the fp32 MFMA cannot overlap vector-ALU work);
# canberra_f32.hip with LLVM's iterative-ilp scheduler: the counting loop is four independent packed-f16 chains per
# dimension pair, and the default scheduler leaves 156 hazard s_nop in it (none with this one): kernel 45.4 -> 40.8 ms at
# 100k x 100k, 3.79 -> 3.43 s at 1M x 1M;
# the same scheduler for l2_topk.hip (hit path and filter are plain vector code around the fenced MFMA chains): 1M x 1M
# kernel 755 -> 735 ms;
# keep MFMA accumulators in arch VGPRs so the C-in (||y||^2 block) needs no
# v_accvgpr_write and the filter reads the scores without v_accvgpr_read (see l2_topk.hip)
FILE_FLAGS = {"l2_topk.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form", "-fno-honor-nans", "-mllvm", "-amdgpu-sched-strategy=iterative-ilp"], "l2q_topk.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form"],
              # l2c_topk.hip: its scores are finite or +inf by construction (pack_ctiles_kernel<.,.,1>), so the filter's minimum tree
              # needs no NaN canonicalisation (two v_max per row-block otherwise)
              "l2c_topk.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form", "-fno-honor-nans"],
              "canberra_f32.hip": ["-mllvm", "-amdgpu-sched-strategy=iterative-ilp"]}
HEADERS = [os.path.join(CSRC, "knn_common.h"), os.path.join(CSRC, "topk_lists.h"), os.path.join(CSRC, "launch.h"),
           os.path.join(CSRC, "host_common.h"), os.path.join(CSRC, "de_exact.h"), os.path.join(CSRC, "comm.h"), os.path.join(CSRC, "index.h"), os.path.join(CSRC, "local_seeds.h"), os.path.join(CSRC, "bucket_order.h"), os.path.join(CSRC, "two_level_verdict.h"), os.path.join(CSRC, "l2c_slots.h"), os.path.join(CSRC, "l2c_window.h"), os.path.join(CSRC, "bucket_skip.h"), os.path.join(CSRC, "simple_graph.h"), os.path.join(CSRC, "row_chunks.h"), os.path.join(CSRC, "umap_common.h"), os.path.join(HERE, "..", "include", "nabo_knn.h"), os.path.join(HERE, "..", "include", "nabo_graph.h"),
           os.path.join(HERE, "..", "include", "nabo_cluster.h"), os.path.join(HERE, "..", "include", "nabo_de.h"),
           os.path.join(HERE, "..", "include", "nabo_pca.h"), os.path.join(HERE, "..", "include", "nabo_pca_fit.h"),
           os.path.join(HERE, "..", "include", "nabo_qc.h"), os.path.join(HERE, "..", "include", "nabo_layout.h"),
           os.path.join(HERE, "..", "include", "nabo_umap.h"), os.path.join(HERE, "..", "include", "nabo_umap_transform.h"),
           os.path.join(HERE, "..", "include", "nabo_community.h"), os.path.join(HERE, "..", "include", "nabo_agglom.h"),
           os.path.join(HERE, "..", "include", "nabo_potential.h"), os.path.join(HERE, "..", "include", "nabo_bundle.h"),
           os.path.join(CSRC, "bundle_view.h"), os.path.join(HERE, "..", "include", "nabo_render.h"),
           os.path.join(CSRC, "mtx_host.h"), os.path.join(HERE, "..", "include", "nabo_ingest.h"),
           os.path.join(CSRC, "mtx_stages.h"), os.path.join(CSRC, "counts_host.h"), os.path.join(HERE, "..", "include", "nabo_counts.h"),
           os.path.join(CSRC, "csv_number.h"), os.path.join(CSRC, "csv_host.h"), os.path.join(HERE, "..", "include", "nabo_csv.h")]
ARCH = "gfx950"
FLAGS = ["-O3", "--offload-arch=" + ARCH, "-fPIC", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
         "-Wall", "-Wno-unused-function", "-Wno-inline-asm"]


def hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found; libnabo_knn.so cannot be built")
    return exe


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _compile(args):
    src, obj, verbose, extra = args
    cmd = [hipcc()] + FLAGS + extra + ["-c", src, "-o", obj]
    if verbose:
        print(" ".join(cmd), flush=True)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    if r.returncode != 0 or verbose:
        sys.stderr.write(r.stdout)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed on %s" % src)
    return obj


def build(force=False, verbose=False, extra=None, out=None):
    """out: build ANOTHER copy of the library (another commit's sources, extra compiler flags) into that file, with its own
    object directory -- a parent / branch A/B loads it through NABO_KNN_SO; the product's libnabo_knn.so is never touched."""
    extra = list(extra or [])
    global SO
    so_saved = SO
    objdir = os.path.join(CSRC, "build")
    if out:
        SO = os.path.abspath(out)
        objdir = os.path.join(CSRC, "build_" + os.path.splitext(os.path.basename(out))[0])
    try:
        return _build(force, verbose, extra, objdir)
    finally:
        SO = so_saved


def _build(force, verbose, extra, objdir):
    os.makedirs(objdir, exist_ok=True)
    jobs, objs = [], []
    for s in SOURCES:
        src = os.path.join(CSRC, s)
        obj = os.path.join(objdir, s.replace(".hip", ".o"))
        objs.append(obj)
        if force or _stale(obj, [src] + HEADERS + [os.path.abspath(__file__)]):
            jobs.append((src, obj, verbose, extra + FILE_FLAGS.get(s, [])))
    if jobs:
        with concurrent.futures.ThreadPoolExecutor(max_workers=min(len(jobs), 6)) as ex:
            list(ex.map(_compile, jobs))
    if jobs or force or _stale(SO, objs):
        cmd = [hipcc(), "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", SO] + objs + ["-ldl", "-lpthread"]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return SO


if __name__ == "__main__":
    # python -m nabo_amd._build [--force] [--verbose] [--out other.so -DFLAG ... [-- more hipcc flags]]
    args = sys.argv[1:]
    out = args[args.index("--out") + 1] if "--out" in args else None
    extra = [a for a in args if a.startswith("-D")] + (args[args.index("--") + 1:] if "--" in args else [])
    print(build(force="--force" in args, verbose="--verbose" in args, extra=extra, out=out))
