"""Builds libmi355_retrieval.so (HIP kernels + C ABI) for gfx950 with hipcc, in-tree.

hipcc cross-compiles without a GPU, so this runs in the build container; the resulting .so is
git-ignored but travels to the GPU box with the tree.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libmi355_retrieval.so")
SOURCES = ["api_state.hip", "api_schedule.hip", "api_gallery.hip", "api_file.hip", "api_entry.hip", "api_aux.hip", "api_options.hip",
           "api_online.hip", "api_range.hip", "api_filter.hip", "api_group.hip", "api_l2.hip", "api_refine.hip", "api_remove.hip", "api_hamming.hip", "api_components.hip", "api_lsh.hip", "api_pq.hip", "api_pq_train.hip", "api_kmeans.hip", "kmeans.hip", "api_pq_wide.hip",
           "api_ivfpq.hip", "api_ivfflat.hip", "api_minkowski.hip", "minkowski.hip", "api_minkowski_range.hip", "minkowski_range.hip", "api_graph.hip", "api_pq_graph.hip", "api_forest.hip", "forest_project.hip", "forest_build.hip", "forest_search.hip", "graph_search.hip", "graph_build.hip", "pq_graph_search.hip", "ivfpq.hip", "ivfpq_residual.hip", "ivfflat.hip",
           "ingest.hip", "gemm_select.hip", "stream_select.hip", "select.hip", "range_select.hip", "csr_order.hip", "filter_select.hip", "group_select.hip", "row_remove.hip", "exact_score.hip", "aqe.hip",
           "synth.hip", "l2_metric.hip", "refine.hip", "hamming.hip", "hamming_range.hip", "components.hip", "lsh.hip", "pq.hip", "pq_train.hip", "pq_wide.hip", "pq_remove.hip", "dense.hip", "diffusion.hip", "whiten.hip", "scatter.hip", "desc_tail.hip", "kr_rerank.hip"]
FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-Wno-unused-value", "-Wno-unused-result"]


def _sources():
    return [s for s in SOURCES if os.path.exists(os.path.join(CSRC, s))]


def needs_build():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [
        os.path.join(os.path.dirname(HERE), "include", "mi355_retrieval.h")]
    return any(os.path.getmtime(p) > t for p in deps)


def build(force=False, verbose=True):
    if not force and not needs_build():
        return LIB
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    srcs = _sources()

    def compile_one(src):
        obj = os.path.join(objdir, src.replace(".hip", ".o"))
        cmd = [hipcc, *FLAGS, *os.environ.get("HIPCC_EXTRA", "").split(), "-c", os.path.join(CSRC, src), "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed for %s:\n%s" % (src, r.stderr[-4000:]))
        return obj

    with ThreadPoolExecutor(max_workers=4) as ex:
        objs = list(ex.map(compile_one, srcs))
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB, *objs]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("link failed:\n" + r.stderr[-4000:])
    if verbose:
        print("built", LIB, file=sys.stderr)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
