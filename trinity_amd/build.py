"""In-tree build of the native libraries (explicit hipcc / g++; no JIT cache, so the .so files travel with the
repo snapshot to the GPU box)."""
import os
import shutil
import subprocess

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
LIB_HIP = os.path.join(PKG, "libtrinity_hip.so")
LIB_HOST = os.path.join(PKG, "libtrinity_host.so")
HIP_SRCS = [os.path.join(PKG, "csrc", n) for n in ("trinity_hip.hip", "commit_sort.hip", "filtered_kernels.hip")]  # (filtered_kernels.hip: csrc/k_filter.hpp)
HOST_SRCS = [os.path.join(PKG, "csrc", "host", "synth.cpp"), os.path.join(PKG, "csrc", "host", "plan_host.cpp")]


def _newer(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _deps(srcs):
    out = list(srcs) + [os.path.join(ROOT, "include", "trinity_hip.h")]
    for d in {os.path.dirname(s) for s in srcs} | {os.path.join(PKG, "csrc")}:  # (the host tools include the planner's headers of csrc/)
        out += [os.path.join(d, f) for f in os.listdir(d) if f.endswith((".hpp", ".h", ".cuh"))]
    return out


def hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found")


def build_hip(force=False):
    if force or _newer(LIB_HIP, _deps(HIP_SRCS) + [os.path.join(PKG, "csrc", "host", n) for n in ("result_rows.hpp", "isect_rows.hpp", "perc_lower.hpp", "facet_rows.hpp", "order_rows.hpp", "stats_rows.hpp", "column_pred.hpp")]):  # (read_side.hpp's host transforms, isect_side.hpp's replay, perc_side.hpp's lowering, read_side.hpp's sum of a collection's facet rows, split of an ordered row's keys, combine of a collection's stats rows, colfilter_side.hpp's validation of column predicates)
        cmd = [hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-Wno-unused-value", "-o", LIB_HIP] + HIP_SRCS + ["-ldl"]
        subprocess.run(cmd, check=True)
    return LIB_HIP


def build_host(force=False):
    if force or _newer(LIB_HOST, _deps(HOST_SRCS)):
        cmd = ["g++", "-O3", "-std=c++17", "-shared", "-fPIC", "-pthread", "-o", LIB_HOST] + HOST_SRCS
        subprocess.run(cmd, check=True)
    return LIB_HOST


MIRROR_TEST_SRC = os.path.join(ROOT, "tests", "cpp", "host_mirror_test.cpp")
MIRROR_TEST_BIN = os.path.join(ROOT, "tests", "cpp", "host_mirror_test")


def build_mirror_test(force=False):
    """The C++ operator surface (csrc/host/trinity_gpu.hpp) compiled into its test driver, linked to libtrinity_hip.so."""
    deps = [MIRROR_TEST_SRC, os.path.join(PKG, "csrc", "host", "trinity_gpu.hpp"), os.path.join(PKG, "csrc", "host", "google_encoder.hpp"), os.path.join(ROOT, "include", "trinity_hip.h")]
    if force or _newer(MIRROR_TEST_BIN, deps):
        build_hip()
        cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-o", MIRROR_TEST_BIN, MIRROR_TEST_SRC, "-L" + PKG, "-ltrinity_hip", "-Wl,-rpath,$ORIGIN/../../trinity_amd"]
        subprocess.run(cmd, check=True)
    return MIRROR_TEST_BIN


MIRROR_WRITE_SRC = os.path.join(ROOT, "tests", "cpp", "host_mirror_write_test.cpp")
MIRROR_WRITE_BIN = os.path.join(ROOT, "tests", "cpp", "host_mirror_write_test")


def build_mirror_write_test(force=False):
    """The write side of the operator surface (csrc/host/trinity_gpu_write.hpp: SegmentIndexSession begin / insert / commit, merge) compiled into its
    driver; in-tree, so that it travels to the GPU box, where tests/test_host_mirror.py runs it."""
    deps = [MIRROR_WRITE_SRC, os.path.join(PKG, "csrc", "host", "trinity_gpu_write.hpp"), os.path.join(PKG, "csrc", "host", "google_encoder.hpp"), os.path.join(ROOT, "include", "trinity_hip.h")]
    if force or _newer(MIRROR_WRITE_BIN, deps):
        build_hip()
        cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", MIRROR_WRITE_BIN, MIRROR_WRITE_SRC, "-L" + PKG, "-ltrinity_hip", "-Wl,-rpath,$ORIGIN/../../trinity_amd"]
        subprocess.run(cmd, check=True)
    return MIRROR_WRITE_BIN


MIRROR_FILTER_SRC = os.path.join(ROOT, "tests", "cpp", "host_mirror_filter_test.cpp")
MIRROR_FILTER_BIN = os.path.join(ROOT, "tests", "cpp", "host_mirror_filter_test")


def build_mirror_filter_test(force=False):
    """exec_query / exec_queries with a DeviceDocumentsFilter (csrc/host/trinity_gpu.hpp) next to the equivalent host filter, compiled into its driver; in-tree,
    like the other two."""
    deps = [MIRROR_FILTER_SRC, os.path.join(PKG, "csrc", "host", "trinity_gpu.hpp"), os.path.join(PKG, "csrc", "host", "google_encoder.hpp"), os.path.join(ROOT, "include", "trinity_hip.h")]
    if force or _newer(MIRROR_FILTER_BIN, deps):
        build_hip()
        cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", MIRROR_FILTER_BIN, MIRROR_FILTER_SRC, "-L" + PKG, "-ltrinity_hip", "-Wl,-rpath,$ORIGIN/../../trinity_amd"]
        subprocess.run(cmd, check=True)
    return MIRROR_FILTER_BIN


MIRROR_WIDE_TERMS_SRC = os.path.join(ROOT, "tests", "cpp", "host_mirror_wide_terms_test.cpp")
MIRROR_WIDE_TERMS_BIN = os.path.join(ROOT, "tests", "cpp", "host_mirror_wide_terms_test")


def build_mirror_wide_terms_test(force=False):
    """exec_query's default mode on queries of more than 16 terms (csrc/host/trinity_gpu.hpp: option rich_max_terms, the _wide result calls) compiled into its driver;
    in-tree, so that it travels to the GPU box, where tests/test_host_mirror_wide_terms.py runs it."""
    deps = [MIRROR_WIDE_TERMS_SRC, os.path.join(PKG, "csrc", "host", "trinity_gpu.hpp"), os.path.join(PKG, "csrc", "host", "google_encoder.hpp"), os.path.join(ROOT, "include", "trinity_hip.h")]
    if force or _newer(MIRROR_WIDE_TERMS_BIN, deps):
        build_hip()
        cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", MIRROR_WIDE_TERMS_BIN, MIRROR_WIDE_TERMS_SRC, "-L" + PKG, "-ltrinity_hip", "-Wl,-rpath,$ORIGIN/../../trinity_amd"]
        subprocess.run(cmd, check=True)
    return MIRROR_WIDE_TERMS_BIN


MIRROR_HITS_SRC = os.path.join(ROOT, "tests", "cpp", "host_mirror_hits_test.cpp")
MIRROR_HITS_BIN = os.path.join(ROOT, "tests", "cpp", "host_mirror_hits_test")


def build_mirror_hits_test(force=False):
    """PostingsListIterator::materialize_hits, DocWordsSpace and IndexSource::term_hits_at (csrc/host/trinity_gpu.hpp: tri_decode_hits / tri_decode_hits_at) compiled
    into their driver; in-tree, so that it travels to the GPU box, where tests/test_host_mirror_hits.py runs it."""
    deps = [MIRROR_HITS_SRC, os.path.join(PKG, "csrc", "host", "trinity_gpu.hpp"), os.path.join(PKG, "csrc", "host", "google_encoder.hpp"), os.path.join(ROOT, "include", "trinity_hip.h")]
    if force or _newer(MIRROR_HITS_BIN, deps):
        build_hip()
        cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", MIRROR_HITS_BIN, MIRROR_HITS_SRC, "-L" + PKG, "-ltrinity_hip", "-Wl,-rpath,$ORIGIN/../../trinity_amd"]
        subprocess.run(cmd, check=True)
    return MIRROR_HITS_BIN


MIRROR_RANK_SRC = os.path.join(ROOT, "tests", "cpp", "host_mirror_rank_test.cpp")
MIRROR_RANK_BIN = os.path.join(ROOT, "tests", "cpp", "host_mirror_rank_test")


def build_mirror_rank_test(force=False):
    """exec_query's default mode with a ProximityRanker (csrc/host/trinity_gpu.hpp: ranked on the device through tri_batch_set_ranker, and through the per-match replay)
    compiled into its driver; in-tree, so that it travels to the GPU box, where tests/test_host_mirror_rank.py runs it."""
    deps = [MIRROR_RANK_SRC, os.path.join(PKG, "csrc", "host", "trinity_gpu.hpp"), os.path.join(PKG, "csrc", "host", "google_encoder.hpp"), os.path.join(ROOT, "include", "trinity_hip.h")]
    if force or _newer(MIRROR_RANK_BIN, deps):
        build_hip()
        cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", MIRROR_RANK_BIN, MIRROR_RANK_SRC, "-L" + PKG, "-ltrinity_hip", "-Wl,-rpath,$ORIGIN/../../trinity_amd"]
        subprocess.run(cmd, check=True)
    return MIRROR_RANK_BIN


MIRROR_COLLECTION_SRC = os.path.join(ROOT, "tests", "cpp", "host_mirror_collection_test.cpp")
MIRROR_COLLECTION_BIN = os.path.join(ROOT, "tests", "cpp", "host_mirror_collection_test")


def build_mirror_collection_test(force=False):
    """IndexSourcesCollection, exec_query's collection form and ProximityRanker::blend (csrc/host/trinity_gpu.hpp) compiled into their driver; in-tree, so that it
    travels to the GPU box, where tests/test_host_mirror_collection.py runs it."""
    deps = [MIRROR_COLLECTION_SRC, os.path.join(PKG, "csrc", "host", "trinity_gpu.hpp"), os.path.join(PKG, "csrc", "host", "google_encoder.hpp"), os.path.join(ROOT, "include", "trinity_hip.h")]
    if force or _newer(MIRROR_COLLECTION_BIN, deps):
        build_hip()
        cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", MIRROR_COLLECTION_BIN, MIRROR_COLLECTION_SRC, "-L" + PKG, "-ltrinity_hip", "-Wl,-rpath,$ORIGIN/../../trinity_amd"]
        subprocess.run(cmd, check=True)
    return MIRROR_COLLECTION_BIN


MIRROR_ISECT_SRC = os.path.join(ROOT, "tests", "cpp", "host_mirror_isect_test.cpp")
MIRROR_ISECT_BIN = os.path.join(ROOT, "tests", "cpp", "host_mirror_isect_test")


def build_mirror_isect_test(force=False):
    """Trinity::intersect on the operator surface (csrc/host/trinity_gpu.hpp: intersect_impl / intersect over a source and over a collection, through tri_isect_run)
    compiled into its driver; in-tree, so that it travels to the GPU box, where tests/test_host_mirror_isect.py runs it."""
    deps = [MIRROR_ISECT_SRC, os.path.join(PKG, "csrc", "host", "trinity_gpu.hpp"), os.path.join(PKG, "csrc", "host", "google_encoder.hpp"), os.path.join(ROOT, "include", "trinity_hip.h")]
    if force or _newer(MIRROR_ISECT_BIN, deps):
        build_hip()
        cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", MIRROR_ISECT_BIN, MIRROR_ISECT_SRC, "-L" + PKG, "-ltrinity_hip", "-Wl,-rpath,$ORIGIN/../../trinity_amd"]
        subprocess.run(cmd, check=True)
    return MIRROR_ISECT_BIN


MIRROR_PERC_SRC = os.path.join(ROOT, "tests", "cpp", "host_mirror_perc_test.cpp")
MIRROR_PERC_BIN = os.path.join(ROOT, "tests", "cpp", "host_mirror_perc_test")


def build_mirror_perc_test(force=False):
    """The percolator of the operator surface (csrc/host/trinity_gpu.hpp: percolator_query, its document proxy, PercolatorSet over tri_perc_create / tri_perc_match)
    compiled into its driver; in-tree, so that it travels to the GPU box, where tests/test_host_mirror_perc.py runs it."""
    deps = [MIRROR_PERC_SRC, os.path.join(ROOT, "tests", "cpp", "perc_case_file.hpp"), os.path.join(PKG, "csrc", "host", "trinity_gpu.hpp"), os.path.join(PKG, "csrc", "host", "google_encoder.hpp"),
            os.path.join(ROOT, "include", "trinity_hip.h")]  # fmt: skip
    if force or _newer(MIRROR_PERC_BIN, deps):
        build_hip()
        cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", MIRROR_PERC_BIN, MIRROR_PERC_SRC, "-L" + PKG, "-ltrinity_hip", "-Wl,-rpath,$ORIGIN/../../trinity_amd"]
        subprocess.run(cmd, check=True)
    return MIRROR_PERC_BIN


MIRROR_FACETS_SRC = os.path.join(ROOT, "tests", "cpp", "host_mirror_facets_test.cpp")
MIRROR_FACETS_BIN = os.path.join(ROOT, "tests", "cpp", "host_mirror_facets_test")


def build_mirror_facets_test(force=False):
    """FacetCounter and DeviceColumn of the operator surface (csrc/host/trinity_gpu.hpp: counted on the device through tri_batch_set_facets / tri_batch_facets, and through
    the replay) compiled into their driver; in-tree, so that it travels to the GPU box, where tests/test_host_mirror_facets.py runs it."""
    deps = [MIRROR_FACETS_SRC, os.path.join(PKG, "csrc", "host", "trinity_gpu.hpp"), os.path.join(PKG, "csrc", "host", "facet_rows.hpp"), os.path.join(PKG, "csrc", "host", "google_encoder.hpp"),
            os.path.join(ROOT, "include", "trinity_hip.h")]  # fmt: skip
    if force or _newer(MIRROR_FACETS_BIN, deps):
        build_hip()
        cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", MIRROR_FACETS_BIN, MIRROR_FACETS_SRC, "-L" + PKG, "-ltrinity_hip", "-Wl,-rpath,$ORIGIN/../../trinity_amd"]
        subprocess.run(cmd, check=True)
    return MIRROR_FACETS_BIN


MIRROR_ORDER_SRC = os.path.join(ROOT, "tests", "cpp", "host_mirror_order_test.cpp")
MIRROR_ORDER_BIN = os.path.join(ROOT, "tests", "cpp", "host_mirror_order_test")


def build_mirror_order_test(force=False):
    """ColumnOrder of the operator surface (csrc/host/trinity_gpu.hpp: selected on the device through tri_batch_set_order / tri_batch_ordered, and through the replay)
    compiled into its driver; in-tree, so that it travels to the GPU box, where tests/test_host_mirror_order.py runs it."""
    deps = [MIRROR_ORDER_SRC, os.path.join(PKG, "csrc", "host", "trinity_gpu.hpp"), os.path.join(PKG, "csrc", "host", "order_rows.hpp"), os.path.join(PKG, "csrc", "host", "google_encoder.hpp"),
            os.path.join(ROOT, "include", "trinity_hip.h")]  # fmt: skip
    if force or _newer(MIRROR_ORDER_BIN, deps):
        build_hip()
        cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", MIRROR_ORDER_BIN, MIRROR_ORDER_SRC, "-L" + PKG, "-ltrinity_hip", "-Wl,-rpath,$ORIGIN/../../trinity_amd"]
        subprocess.run(cmd, check=True)
    return MIRROR_ORDER_BIN


MIRROR_STATS_SRC = os.path.join(ROOT, "tests", "cpp", "host_mirror_stats_test.cpp")
MIRROR_STATS_BIN = os.path.join(ROOT, "tests", "cpp", "host_mirror_stats_test")


def build_mirror_stats_test(force=False):
    """StatsCounter of the operator surface (csrc/host/trinity_gpu.hpp: aggregated on the device through tri_batch_set_stats / tri_batch_stats, and through the replay)
    compiled into its driver; in-tree, so that it travels to the GPU box, where tests/test_host_mirror_stats.py runs it."""
    deps = [MIRROR_STATS_SRC, os.path.join(PKG, "csrc", "host", "trinity_gpu.hpp"), os.path.join(PKG, "csrc", "host", "stats_rows.hpp"), os.path.join(PKG, "csrc", "host", "google_encoder.hpp"),
            os.path.join(ROOT, "include", "trinity_hip.h")]  # fmt: skip
    if force or _newer(MIRROR_STATS_BIN, deps):
        build_hip()
        cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", MIRROR_STATS_BIN, MIRROR_STATS_SRC, "-L" + PKG, "-ltrinity_hip", "-Wl,-rpath,$ORIGIN/../../trinity_amd"]
        subprocess.run(cmd, check=True)
    return MIRROR_STATS_BIN


MIRROR_COLFILTER_SRC = os.path.join(ROOT, "tests", "cpp", "host_mirror_colfilter_test.cpp")
MIRROR_COLFILTER_BIN = os.path.join(ROOT, "tests", "cpp", "host_mirror_colfilter_test")


def build_mirror_colfilter_test(force=False):
    """ColumnPredicateFilter of the operator surface (csrc/host/trinity_gpu.hpp: an IndexDocumentsFilter over DeviceColumns, built on the device through
    tri_filters_from_columns, and answered on the host through column_pred.hpp) compiled into its driver; in-tree, so that it travels to the GPU box, where
    tests/test_host_mirror_colfilter.py runs it."""
    deps = [MIRROR_COLFILTER_SRC, os.path.join(PKG, "csrc", "host", "trinity_gpu.hpp"), os.path.join(PKG, "csrc", "host", "column_pred.hpp"), os.path.join(PKG, "csrc", "host", "google_encoder.hpp"),
            os.path.join(ROOT, "include", "trinity_hip.h")]  # fmt: skip
    if force or _newer(MIRROR_COLFILTER_BIN, deps):
        build_hip()
        cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", MIRROR_COLFILTER_BIN, MIRROR_COLFILTER_SRC, "-L" + PKG, "-ltrinity_hip", "-Wl,-rpath,$ORIGIN/../../trinity_amd"]
        subprocess.run(cmd, check=True)
    return MIRROR_COLFILTER_BIN


def build_all(force=False):
    return (build_hip(force), build_host(force), build_mirror_test(force), build_mirror_write_test(force), build_mirror_filter_test(force), build_mirror_wide_terms_test(force),
            build_mirror_hits_test(force), build_mirror_rank_test(force), build_mirror_collection_test(force), build_mirror_isect_test(force), build_mirror_perc_test(force), build_mirror_facets_test(force), build_mirror_order_test(force),
            build_mirror_stats_test(force), build_mirror_colfilter_test(force))


def kernels_stamp():
    """SHA-256 (16 hex digits) over the device sources (csrc/*.hip, csrc/*.hpp): what a committed profile is stamped with — bench.py quotes
    profiles/pmc_latest.json's traffic only while the stamp it carries is that of the kernels it runs."""
    import hashlib

    h = hashlib.sha256()
    d = os.path.join(PKG, "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".hpp")):
            with open(os.path.join(d, f), "rb") as fh:
                h.update(f.encode() + b"\0" + fh.read())
    return h.hexdigest()[:16]
