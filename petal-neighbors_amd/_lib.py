"""ctypes binding of libpetal_mi355x.so (include/petal_mi355x.h).

The library is the product: if it is missing or does not export a declared
symbol this module raises -- there is no Python/NumPy fallback.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# PN_LIBRARY_PATH: a diagnostic build (build.py with PN_DIAG_FLAGS writes libpetal_mi355x_diag.so) for tools/ only
LIB_PATH = os.environ.get("PN_LIBRARY_PATH") or os.path.join(_HERE, "libpetal_mi355x.so")

PN_OK, PN_ERR_EMPTY, PN_ERR_NOT_CONTIGUOUS, PN_ERR_INVALID, PN_ERR_DEVICE, PN_ERR_NOMEM, \
    PN_ERR_UNSUPPORTED, PN_ERR_EMPTY_MATRIX, PN_ERR_COMM = range(9)
PN_COMM_ID_BYTES = 128
PN_ENGINE_AUTO, PN_ENGINE_EXACT, PN_ENGINE_MFMA, PN_ENGINE_BF16 = 0, 1, 2, 3
PN_OPT_ENGINE, PN_OPT_SEGMENTS, PN_OPT_INDEX_BASE, PN_OPT_PROFILE, PN_OPT_FILTER_SLOTS = 1, 2, 3, 4, 5
PN_OPT_MFMA_STRUCTURE = 6
PN_OPT_EXCHANGE_ALWAYS = 7
PN_OPT_SHARED_THRESHOLDS = 8
PN_OPT_BF16_WAVES = 9
PN_OPT_SEED_MODEL = 10
PN_OPT_DBSCAN_PIECE = 11
PN_OPT_MST_BATCH = 12
PN_OPT_OPTICS_PIECE = 13
PN_OPT_KDE_PIECE = 14
PN_OPT_MS_PIECE = 15
PN_OPT_KMEANS_FILTER = 16
PN_KDE_GAUSSIAN, PN_KDE_TOPHAT, PN_KDE_EPANECHNIKOV, PN_KDE_EXPONENTIAL, PN_KDE_LINEAR = 0, 1, 2, 3, 4
PN_RADIUS_SORTED = 1
PN_SELF_INCLUDE = 2
PN_MS_SEED_ROWS = 4
PN_MS_ORPHANS = 8
PN_KNN_WEIGHT_DISTANCE = 1


class PnInfo(C.Structure):
    _fields_ = [("n_points", C.c_uint64), ("dim", C.c_uint64), ("row_stride_device", C.c_uint64),
                ("elem_bytes", C.c_int32), ("device", C.c_int32), ("mfma_eligible", C.c_int32),
                ("bf16_eligible", C.c_int32), ("bf16_layout", C.c_int32), ("seed_model", C.c_int32)]


class PnStats(C.Structure):
    _fields_ = [("queries", C.c_uint64), ("fallback_queries", C.c_uint64), ("candidates", C.c_uint64),
                ("hot_launches", C.c_uint64), ("hot_ms", C.c_double), ("last_call_ms", C.c_double),
                ("radius_results", C.c_uint64), ("evaluations", C.c_uint64),
                ("shard_ms", C.c_double), ("exchange_ms", C.c_double), ("reserved", C.c_uint64 * 1)]


class PnShardedInfo(C.Structure):
    _fields_ = [("n_points", C.c_uint64), ("dim", C.c_uint64), ("local_first_row", C.c_uint64),
                ("local_rows", C.c_uint64), ("n_shards", C.c_int32), ("world", C.c_int32),
                ("local_shards", C.c_int32), ("rank", C.c_int32), ("mfma_eligible", C.c_int32),
                ("bf16_eligible", C.c_int32)]


_sz, _ssz, _i, _vp, _u64, _cu, _d = C.c_size_t, C.c_ssize_t, C.c_int, C.c_void_p, C.c_uint64, C.c_uint, C.c_double
_u64p, _ip, _vpp = C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.POINTER(C.c_void_p)
_R, _RP = "real", "real*"  # the handle's element type and a pointer to it: c_float / c_double by suffix

# queries / centres / seeds on the host (rows, nq, qc, stride) and in HBM
_QH, _QD = [_vp, _vp, _sz, _sz, _ssz], [_vp, _vp, _sz, _sz, _sz]
# the CSR results of the radius searches: host (offsets, idx**, dist**), device (offsets, idx, dist, capacity, total, stream)
_CSR_H, _CSR_D = [_vp, _vpp, _vpp], [_vp, _vp, _vp, _sz, _vp, _vp]
_CREATE = [_vp, _sz, _sz, _ssz, _ssz, _i, _vpp]
_SH_CREATE = [_vp, _sz, _sz, _ssz, _ssz, _ip, _i, _vpp]
_PAIRWISE = [_vp, _sz, _sz, _ssz, _i, _vp]

# stem -> (restype, argtypes): declared once, expanded to stem_f32 and stem_f64 with _R / _RP as the suffix's type
PAIRED = {
    "pn_index_create": (_i, _CREATE),
    "pn_index_create_cosine": (_i, _CREATE),
    "pn_pairwise_device": (_i, [_vp, _sz, _sz, _sz, _i, _vp, _vp]),
    "pn_index_create_device": (_i, [_vp, _sz, _sz, _sz, _i, _vp, _vpp]),
    "pn_query": (_i, _QH + [_sz, _vp, _vp]),
    "pn_query_device": (_i, _QD + [_sz, _vp, _vp, _vp]),
    "pn_query_nearest": (_i, _QH + [_vp, _vp]),
    "pn_query_radius": (_i, _QH + [_R, _vp, _vpp]),
    "pn_query_radius_device": (_i, _QD + [_R, _vp, _vp, _sz, _vp, _vp]),
    "pn_query_radius_with_distance": (_i, _QH + [_R, _cu] + _CSR_H),
    "pn_query_radius_with_distance_device": (_i, _QD + [_R, _cu] + _CSR_D),
    "pn_query_self": (_i, [_vp, _sz, _cu, _vp, _vp]),
    "pn_query_self_device": (_i, [_vp, _sz, _cu, _vp, _vp, _vp]),
    "pn_query_radius_self": (_i, [_vp, _R, _cu] + _CSR_H),
    "pn_query_radius_self_device": (_i, [_vp, _R, _cu] + _CSR_D),
    "pn_query_radii": (_i, _QH + [_vp, _cu] + _CSR_H),
    "pn_query_radii_device": (_i, _QD + [_vp, _cu] + _CSR_D),
    "pn_query_radii_self": (_i, [_vp, _vp, _cu] + _CSR_H),
    "pn_query_radii_self_device": (_i, [_vp, _vp, _cu] + _CSR_D),
    "pn_dbscan": (_i, [_vp, _R, _sz, _cu] + [_vp] * 3),
    "pn_dbscan_device": (_i, [_vp, _R, _sz, _cu] + [_vp] * 4),
    "pn_mst": (_i, [_vp, _vp, _cu] + [_vp] * 4),
    "pn_mst_device": (_i, [_vp, _vp, _cu] + [_vp] * 5),
    "pn_linkage": (_i, [_vp] * 4 + [_cu] + [_vp] * 4),
    "pn_linkage_device": (_i, [_vp] * 4 + [_cu] + [_vp] * 6),
    "pn_hdbscan": (_i, [_vp, _sz, _sz, _cu] + [_vp] * 3),
    "pn_hdbscan_device": (_i, [_vp, _sz, _sz, _cu] + [_vp] * 4),
    "pn_lof": (_i, [_vp, _sz, _cu] + [_vp] * 3),
    "pn_lof_device": (_i, [_vp, _sz, _cu] + [_vp] * 4),
    "pn_lof_score": (_i, _QH + [_sz, _vp, _vp, _cu, _vp]),
    "pn_lof_score_device": (_i, _QD + [_sz, _vp, _vp, _cu, _vp, _vp]),
    "pn_knn_classify": (_i, _QH + [_sz, _vp, _sz, _cu, _vp, _vp]),
    "pn_knn_classify_device": (_i, _QD + [_sz, _vp, _sz, _cu] + [_vp] * 3),
    "pn_knn_classify_self": (_i, [_vp, _sz, _vp, _sz, _cu, _vp, _vp]),
    "pn_knn_classify_self_device": (_i, [_vp, _sz, _vp, _sz, _cu] + [_vp] * 3),
    "pn_knn_regress": (_i, _QH + [_sz, _vp, _sz, _cu, _vp]),
    "pn_knn_regress_device": (_i, _QD + [_sz, _vp, _sz, _cu, _vp, _vp]),
    "pn_knn_regress_self": (_i, [_vp, _sz, _vp, _sz, _cu, _vp]),
    "pn_knn_regress_self_device": (_i, [_vp, _sz, _vp, _sz, _cu, _vp, _vp]),
    "pn_kde": (_i, _QH + [_vp, _sz, _i, _d, _cu] + [_vp] * 3),
    "pn_kde_device": (_i, _QD + [_vp, _sz, _i, _d, _cu] + [_vp] * 4),
    "pn_kde_self": (_i, [_vp, _vp, _sz, _i, _d, _cu] + [_vp] * 3),
    "pn_kde_self_device": (_i, [_vp, _vp, _sz, _i, _d, _cu] + [_vp] * 4),
    "pn_mean_shift": (_i, _QH + [_vp, _sz, _d, _sz, _cu] + [_vp] * 5),
    "pn_mean_shift_device": (_i, _QD + [_vp, _sz, _d, _sz, _cu] + [_vp] * 6),
    "pn_mean_shift_merge": (_i, [_vp, _vp, _sz, _vp, _R, _cu] + [_vp] * 4),
    "pn_mean_shift_merge_device": (_i, [_vp, _vp, _sz, _vp, _R, _cu] + [_vp] * 5),
    "pn_mean_shift_labels": (_i, [_vp, _vp, _sz, _R, _cu, _vp]),
    "pn_mean_shift_labels_device": (_i, [_vp, _vp, _sz, _R, _cu, _vp, _vp]),
    "pn_kmeans_assign": (_i, [_vp, _vp, _sz, _cu] + [_vp] * 3),
    "pn_kmeans_assign_device": (_i, [_vp, _vp, _sz, _cu] + [_vp] * 4),
    "pn_kmeans": (_i, [_vp, _vp, _sz, _d, _sz, _cu] + [_vp] * 7),
    "pn_kmeans_device": (_i, [_vp, _vp, _sz, _d, _sz, _cu] + [_vp] * 8),
    "pn_optics": (_i, [_vp, _sz, _R, _cu] + [_vp] * 4),
    "pn_optics_device": (_i, [_vp, _sz, _R, _cu] + [_vp] * 5),
    "pn_optics_dbscan": (_i, [_vp] * 4 + [_R, _cu, _vp, _vp]),
    "pn_optics_dbscan_device": (_i, [_vp] * 4 + [_R, _cu] + [_vp] * 4),
    "pn_pairwise": (_i, _PAIRWISE),
    "pn_pairwise_cosine": (_i, _PAIRWISE),
    "pn_cosine": (_R, [_vp, _sz, _vp, _sz]),
    "pn_euclidean": (_R, [_vp, _vp, _sz]),
    "pn_reuclidean": (_R, [_vp, _vp, _sz]),
    "pn_rdistance_to_distance": (_R, [_R]),
    "pn_distance_to_rdistance": (_R, [_R]),
    "pn_merge_topk_device": (_i, [_vp, _vp] + [_sz] * 6 + [_vp, _vp, _i, _vp]),
    "pn_tree_radius_of": (_i, [_vp, _u64, _RP]),
    "pn_tree_node_distance_lower_bound": (_i, [_vp, _u64, _u64, _RP]),
    "pn_sharded_create": (_i, _SH_CREATE),
    "pn_sharded_create_cosine": (_i, _SH_CREATE),
    "pn_sharded_create_rank_device": (_i, [_vp, _sz, _sz, _sz, _u64, _i, _i, _vp, _i, _vp, _vpp]),
}
# the sharded handle's searches take the arguments of the single index's
for _stem in ("query", "query_device", "query_radius", "query_radius_device", "query_radius_with_distance",
              "query_radius_with_distance_device", "query_self", "query_self_device", "query_radius_self",
              "query_radius_self_device"):
    PAIRED["pn_sharded_" + _stem] = PAIRED["pn_" + _stem]

# the symbols without an f32 / f64 twin
UNPAIRED = {
    "pn_last_error": (C.c_char_p, []),
    "pn_strerror": (C.c_char_p, [_i]),
    "pn_abi_version": (_i, []),
    "pn_device_count": (_i, [_ip]),
    "pn_index_destroy": (None, [_vp]),
    "pn_index_info": (_i, [_vp, C.POINTER(PnInfo)]),
    "pn_index_set_option": (_i, [_vp, _i, C.c_int64]),
    "pn_index_get_stats": (_i, [_vp, C.POINTER(PnStats), _i]),
    "pn_kmeans_bounds_f32": (_i, [_vp, _vp, _sz, _vp]),
    "pn_free": (None, [_vp]),
    "pn_fill_uniform_device_f32": (_i, [_vp, _u64, _u64, _u64, _i, _vp]),
    "pn_bf16_bounds_f32": (_i, _QH + [_sz, _vp, _vp, _vp]),
    "pn_bf16_selftest": (_i, [_i, _vp]),
    "pn_debug_seed_model_feedback": (_i, [_vp, _i, _u64, _u64, _vp]),
    "pn_tree_num_nodes": (_i, [_vp, _u64p]),
    "pn_tree_children_of": (_i, [_vp, _u64, _ip, _u64p, _u64p]),
    "pn_tree_points_of": (_i, [_vp, _u64, C.POINTER(_u64p), _u64p]),
    "pn_tree_compare_nodes": (_i, [_vp, _u64, _u64, _ip]),
    "pn_tree_centroid_of": (_i, [_vp, _u64, _vp]),
    "pn_comm_unique_id": (_i, [_vp]),
    "pn_sharded_destroy": (None, [_vp]),
    "pn_sharded_info": (_i, [_vp, C.POINTER(PnShardedInfo)]),
    "pn_sharded_set_option": (_i, [_vp, _i, C.c_int64]),
    "pn_sharded_get_stats": (_i, [_vp, C.POINTER(PnStats), _i]),
}

REAL = {"f32": C.c_float, "f64": C.c_double}  # suffix -> the ctypes scalar of the element type


def _expand(t, real):
    return real if t is _R else C.POINTER(real) if t is _RP else t


# every symbol include/petal_mi355x.h declares: name -> (restype, argtypes)
SIGNATURES = dict(UNPAIRED)
for _stem, (_res, _args) in PAIRED.items():
    for _sfx, _real in REAL.items():
        SIGNATURES[f"{_stem}_{_sfx}"] = (_expand(_res, _real), [_expand(t, _real) for t in _args])

_lib = None


class LibraryMissing(RuntimeError):
    pass


def lib():
    """Load the HIP library. Raises LibraryMissing loudly; never falls back."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LibraryMissing(
            f"{LIB_PATH} is missing: build it with `python petal-neighbors_amd/build.py` "
            "(or __graft_entry__.build()). petal_neighbors_amd has no CPU fallback.")
    try:
        # PyTorch-ROCm bundles its own libamdhip64.so.7; it must be the HIP runtime already in
        # the process when ours is bound, or two runtimes would fight over the device.
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            f = getattr(L, name)
        except AttributeError as e:
            # PN_LIBRARY_OLDER=1 (tools/ only, next to PN_LIBRARY_PATH): an older build measured against this one -- a
            # symbol it does not export stays unbound, and a call of it raises AttributeError
            if os.environ.get("PN_LIBRARY_OLDER") == "1" and os.environ.get("PN_LIBRARY_PATH"):
                continue
            raise LibraryMissing(f"{LIB_PATH} does not export {name}") from e
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


def last_error() -> str:
    return lib().pn_last_error().decode("utf-8", "replace")
