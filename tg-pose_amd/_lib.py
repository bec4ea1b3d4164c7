"""ctypes binding of libtgpose_hip.so (the C ABI declared in include/tgpose.h).

There is NO fallback: if the library is missing or a call fails, this raises.  The product path
never routes through the CPU oracle or through torch ops for the hot layers.
"""
import ctypes
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libtgpose_hip.so")

c_int, c_i64, c_f32, c_vp = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p


class GemmArgs(ctypes.Structure):
    """struct tgp_gemm_args (include/tgpose.h)"""
    _fields_ = [
        ("A", c_vp), ("lda", c_int),
        ("W", c_vp), ("ldw", c_int),
        ("C", c_vp), ("ldc", c_int),
        ("M", c_int), ("N", c_int), ("K", c_int),
        ("bias", c_vp),
        ("rowbias", c_vp), ("ldrb", c_int),
        ("rows_per_obj", c_int),
        ("res1", c_vp), ("ldr1", c_int),
        ("res2", c_vp), ("ldr2", c_int),
        ("scale", c_vp),
        ("shift", c_vp),
        ("act", c_int),
        ("slope", c_f32),
        ("colmax_keys", c_vp), ("ldcm", c_int),
        ("slope_vec", c_vp),
        ("cm_cols", c_int), ("c_col0", c_int),
        ("batch", c_int),
        ("batch_stride_a", c_i64), ("batch_stride_w", c_i64), ("batch_stride_c", c_i64),
        ("batch_stride_vec", c_i64), ("batch_stride_colmax", c_i64),
        ("W_split", c_vp), ("ldws", c_int), ("w_split_kind", c_int),
        ("a_scale", c_vp), ("c_scale", c_vp), ("ksplit_chunk", c_int),
        ("gres1", c_vp), ("ldg1", c_int), ("gidx1", c_vp),
        ("gres2", c_vp), ("ldg2", c_int), ("gidx2", c_vp),
        ("epilogue", c_int), ("pred", c_vp),
        ("row_base", c_int),
        ("A_planes", c_vp), ("a_kt", c_int), ("a_amax", c_vp),
        ("W_planes", c_vp), ("w_kt", c_int),
        ("C_planes", c_vp), ("c_kt", c_int), ("cp_col0", c_int), ("c_amax", c_vp),
        ("pp_config", c_int),
        ("range_flag", c_vp),
        ("a_keys", c_int), ("a_wrap", c_int),
        ("C_sigmoid", c_vp),
    ]


# name -> (restype, argtypes); every symbol include/tgpose.h declares
class ConvMaxFusedArgs(ctypes.Structure):
    """struct tgp_conv_max_fused_args (include/tgpose.h)"""
    _fields_ = [
        ("fine", c_vp), ("ldf", c_int), ("K", c_int),
        ("wa_planes", c_vp),
        ("p1", c_vp), ("ldp1", c_int), ("p1_rows", c_int), ("idx1", c_vp),
        ("p2", c_vp), ("ldp2", c_int), ("p2_rows", c_int), ("idx2", c_vp),
        ("bias", c_vp), ("scale", c_vp), ("shift", c_vp), ("slope", ctypes.c_float),
        ("keys", c_vp), ("ldk", c_int),
        ("M", c_int), ("rows_per_obj", c_int), ("C", c_int),
        ("overflow", c_vp),
        ("fine_planes", c_vp), ("fine_kt", c_int), ("fine_amax", c_vp),
    ]


class HeadsFusedArgs(ctypes.Structure):
    """struct tgp_heads_fused_args (include/tgpose.h)"""
    _fields_ = [
        ("fine", c_vp), ("ldf", c_int), ("K", c_int),
        ("wa_planes", c_vp),
        ("p1", c_vp), ("ldp1", c_int), ("idx1", c_vp),
        ("p2", c_vp), ("ldp2", c_int), ("idx2", c_vp),
        ("w2p", c_vp),
        ("bias2", c_vp), ("scale2", c_vp), ("shift2", c_vp),
        ("keys", c_vp),
        ("M", c_int), ("rows_per_obj", c_int), ("B", c_int), ("heads", c_int),
        ("overflow", c_vp),
        ("rows", c_int),
        ("fine_planes", c_vp), ("fine_kt", c_int), ("fine_amax", c_vp),
    ]


class DecFusedArgs(ctypes.Structure):
    """struct tgp_dec_fused_args (include/tgpose.h)"""
    _fields_ = [
        ("h1_planes", c_vp), ("h1_kt", c_int), ("h1_amax", c_vp),
        ("units", c_vp),
        ("vec", (c_vp * 3) * 3),
        ("w5", c_vp), ("b5", c_vp),
        ("map", c_vp), ("rows_per_obj", c_int),
        ("out", c_vp),
        ("flag", c_vp),
        ("M", c_int),
    ]


class HsChainArgs(ctypes.Structure):
    """struct tgp_hs_chain_args (include/tgpose.h)"""
    _fields_ = [
        ("a_planes", c_vp), ("a_kt", c_int), ("a_amax", c_vp),
        ("M", c_int), ("K1", c_int), ("N1", c_int), ("N2", c_int),
        ("units", c_vp),
        ("rowbias", c_vp), ("ldrb", c_int), ("rows_per_obj", c_int),
        ("res1", c_vp), ("ldr1", c_int),
        ("res2", c_vp), ("ldr2", c_int),
        ("scale1", c_vp), ("shift1", c_vp),
        ("relu", c_int),
        ("c1", c_vp), ("ldc1", c_int),
        ("c1_planes", c_vp), ("c1_kt", c_int), ("c1_kt0", c_int), ("c1_amax", c_vp),
        ("bias2", c_vp),
        ("c2", c_vp), ("ldc2", c_int),
        ("flag", c_vp),
    ]


class ProjPlanesArgs(ctypes.Structure):
    """struct tgp_proj_planes_args (include/tgpose.h)"""
    _fields_ = [
        ("a_planes", c_vp), ("a_kt", c_int), ("a_amax", c_vp),
        ("a", c_vp), ("lda", c_int),
        ("M", c_int), ("K", c_int), ("N", c_int),
        ("units", c_vp),
        ("w", c_vp), ("ldw", c_int),
        ("bias", c_vp),
        ("c", c_vp), ("ldc", c_int),
    ]


class DecL1Args(ctypes.Structure):
    """struct tgp_dec_l1_args (include/tgpose.h)"""
    _fields_ = [
        ("fine_planes", c_vp), ("fine_kt", c_int), ("fine_amax", c_vp),
        ("wa_planes", c_vp),
        ("p1", c_vp), ("ldp1", c_int), ("idx1", c_vp),
        ("p2", c_vp), ("ldp2", c_int), ("idx2", c_vp),
        ("bias", c_vp), ("scale", c_vp), ("shift", c_vp),
        ("rowbias", c_vp), ("ldrb", c_int), ("rows_per_obj", c_int),
        ("h1_planes", c_vp), ("h1_kt", c_int), ("h1_amax", c_vp),
        ("flag", c_vp),
        ("M", c_int),
    ]


class RangerTensor(ctypes.Structure):
    """struct tgp_ranger_tensor (include/tgpose.h): one tensor of a tgp_ranger_step launch"""
    _fields_ = [
        ("p", c_vp), ("g", c_vp), ("m", c_vp), ("v", c_vp), ("slow", c_vp),
        ("numel", c_i64),
        ("row_len", c_int), ("flags", c_int),
        ("unit0", c_i64),
        ("beta1", c_f32), ("one_minus_beta1", c_f32), ("beta2", c_f32), ("one_minus_beta2", c_f32),
        ("eps", c_f32), ("weight_decay", c_f32), ("neg_step_lr", c_f32), ("alpha", c_f32),
    ]


class RangerArgs(ctypes.Structure):
    """struct tgp_ranger_args (include/tgpose.h)"""
    _fields_ = [("tensors", c_vp), ("n", c_int), ("units", c_i64)]


RANGER_GC, RANGER_ADAPTIVE, RANGER_LOOKAHEAD = 1, 2, 4


class AugmentArgs(ctypes.Structure):
    """struct tgp_augment_args (include/tgpose.h)"""
    _fields_ = [
        ("B", c_int), ("N", c_int),
        ("pc", c_vp),
        ("draws", c_vp),
        ("R", c_vp), ("t", c_vp), ("s", c_vp), ("mean_shape", c_vp),
        ("sym", c_vp), ("aug_bb", c_vp), ("aug_rt_t", c_vp), ("aug_rt_R", c_vp),
        ("cat_id", c_vp), ("nocs_scale", c_vp),
        ("model_point", c_vp), ("n_model", c_int),
        ("defor", c_vp),
        ("pro_bb", c_f32), ("pro_rt", c_f32), ("pro_bc", c_f32), ("pro_pc", c_f32), ("pc_r", c_f32),
        ("pc_out", c_vp), ("R_out", c_vp), ("t_out", c_vp), ("s_out", c_vp),
        ("flags_out", c_vp),
        ("op", c_vp),
        ("noise", c_vp),
        ("drop_ratio", c_vp), ("drop_u", c_vp), ("boxes", c_vp),
        ("crop_max_try", c_int), ("cutout_max_try", c_int), ("crop_min_points", c_int), ("cutout_min_points", c_int),
        ("view_out", c_vp),
        ("count_out", c_vp),
        ("ld_out", c_int),
    ]


AUGMENT_MAX_POINTS, AUGMENT_MAX_TRY = 2048, 16
AUG_NONE, AUG_JITTER, AUG_CUTOUT, AUG_CROP, AUG_DROPOUT = -1, 0, 1, 2, 3


class PdArgs(ctypes.Structure):
    """struct tgp_pd_args (include/tgpose.h)"""
    _fields_ = [
        ("B", c_int), ("N", c_int),
        ("pcl", c_vp), ("workspace", c_vp),
        ("h1", c_vp), ("h2", c_vp),
        ("counts", c_vp), ("status", c_vp),
        ("tets", c_vp), ("ntet", c_vp),
        ("pdh1", c_vp), ("pdh2", c_vp),
        ("tet_cap", c_int),
    ]


PD_MAX_POINTS, PD_MAX_TETS, PD_MAX_PAIRS, PD_PIXELS = 1024, 8192, 4096, 2500
PD_STATUS = {1: "TGP_PD_ETETS (tetrahedron / simplex storage)", 2: "TGP_PD_ECAVITY (one insertion's cavity)",
             3: "TGP_PD_EWALK (point location did not end)", 4: "TGP_PD_EPAIRS (more than PD_MAX_PAIRS pairs)",
             5: "TGP_PD_ECOLUMNS (H1 column storage)", 6: "TGP_PD_ERANGE (coordinate not finite or below the exact grid)",
             7: "TGP_PD_EFLAT (fewer than 4 affinely independent points)", 8: "TGP_PD_EINTERNAL"}

class GatherSlotsArgs(ctypes.Structure):
    """struct tgp_gather_slots_args (include/tgpose.h)"""
    _fields_ = [("slot_item", c_vp), ("B", c_int), ("D", c_int), ("n", c_int),
                ("src", c_vp * 24), ("dst", c_vp * 24), ("row_words", c_int * 24)]


class RenderArgs(ctypes.Structure):
    """struct tgp_render_args (include/tgpose.h)"""
    _fields_ = [("verts", c_vp), ("faces", c_vp), ("vptr", c_vp), ("fptr", c_vp),
                ("M", c_int), ("n_verts", c_int), ("n_faces", c_int), ("max_verts", c_int), ("max_faces", c_int),
                ("scene_ptr", c_vp), ("inst_mesh", c_vp), ("inst_id", c_vp), ("inst_pose", c_vp), ("camk", c_vp),
                ("S", c_int), ("I", c_int), ("max_scene_inst", c_int), ("H", c_int), ("W", c_int), ("near", c_f32),
                ("workspace", c_vp),
                ("depth", c_vp), ("mask", c_vp), ("z", c_vp), ("face", c_vp), ("visible", c_vp), ("bbox", c_vp), ("dropped", c_vp)]


class MeshSampleArgs(ctypes.Structure):
    """struct tgp_mesh_sample_args (include/tgpose.h)"""
    _fields_ = [("verts", c_vp), ("faces", c_vp), ("vptr", c_vp), ("fptr", c_vp), ("cdf", c_vp),
                ("M", c_int), ("n_verts", c_int), ("n_faces", c_int),
                ("job_mesh", c_vp), ("B", c_int), ("n", c_int),
                ("u", c_vp), ("keys", c_vp), ("seed", ctypes.c_uint64),
                ("normals", c_int), ("f32", c_int),
                ("out", c_vp), ("face", c_vp), ("status", c_vp)]


MESH_SITE, MESH_AREA_CHUNK = 8, 64           # TGP_MESH_SITE, TGP_MESH_AREA_CHUNK
BALL_LEVELS, BALL_THREADS = 10, 1024         # TGP_BALL_LEVELS, TGP_BALL_THREADS
MESH_STATUS = {1: "the mesh's total area is not a positive finite number", 2: "the mesh index or the mesh's rows are outside the set"}
GATHER_SLOTS_MAX, DRAW_MAX_ITEMS, DRAW_MAX_TOTAL = 24, 4096, 65536
SITE_HOST, SITE_BAND, SITE_SEL2K, SITE_SEL1K, SITE_DEFOR, SITE_NOISE, SITE_DROP, SITE_SHUFFLE = range(8)
ITEM_ALIVE, ITEM_NO_DEPTH, ITEM_NO_MASK, ITEM_FEW_POINTS, ITEM_BELOW_26, ITEM_WINDOW = range(6)
c_u64, c_u32, c_f64 = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_double

SIGNATURES = {
    "tgp_version": (c_int, []),
    "tgp_graph_node_counts": (c_int, [c_vp, c_vp]),
    "tgp_knn_max_points": (c_int, []),
    "tgp_knn_max_k": (c_int, []),
    "tgp_center": (c_int, [c_vp, c_int, c_int, c_vp, c_vp, c_vp]),
    "tgp_center_zero": (c_int, [c_vp, c_int, c_int, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "tgp_knn_xyz": (c_int, [c_vp, c_int, c_int, c_int, c_vp, c_vp]),
    "tgp_knn_feat_workspace_bytes": (c_i64, [c_int, c_int, c_int]),
    "tgp_knn_feat": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, c_i64, c_vp]),
    "tgp_knn_feat_form": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, c_i64, c_int, c_vp]),
    "tgp_knn_feat_dirs": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "tgp_nn1": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_vp, c_vp]),
    "tgp_nn1_pair": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp]),
    "tgp_nn1_pair_tail": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_int, c_vp, c_int, c_int, c_vp]),
    "tgp_normalize_dirs": (c_int, [c_vp, c_int, c_vp, c_vp]),
    "tgp_normalize_dirs_bwd": (c_int, [c_vp, c_vp, c_int, c_vp, c_vp]),
    "tgp_gconv_surface_fwd": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_int, c_int, c_vp]),
    "tgp_gconv_hs_fwd": (c_int, [c_vp, c_vp, c_vp, c_int, c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_int, c_vp, c_vp]),
    "tgp_gconv_hs_fwd_dirs": (c_int, [c_vp, c_vp, c_vp, c_int, c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_int, c_vp, c_vp]),
    "tgp_orl_partial_floats": (c_i64, [c_int, c_int, c_int]),
    "tgp_orl_global": (c_int, [c_vp, c_int, c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp]),
    "tgp_orl_rowbias": (c_int, [c_vp, c_int, c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "tgp_orl_rowbias_planes": (c_int, [c_vp, c_int, c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_vp, c_vp]),
    "tgp_orl_rowbias_fused": (c_int, [c_vp, c_int, c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_vp, c_vp, c_vp,
                                      c_vp]),
    "tgp_pool_fwd": (c_int, [c_vp, c_vp, c_int, c_vp, c_int, c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, c_int, c_vp]),
    "tgp_pool_fwd_planes": (c_int, [c_vp, c_vp, c_int, c_vp, c_int, c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, c_int, c_vp, c_int,
                                    c_vp, c_vp]),
    "tgp_gather_rows": (c_int, [c_vp, c_int, c_vp, c_int, c_int, c_int, c_int, c_vp, c_int, c_vp]),
    "tgp_fill_tail": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_vp, c_int, c_int, c_vp]),
    "tgp_split_bf16": (c_int, [c_vp, c_int, c_int, c_int, c_vp, c_int, c_vp]),
    "tgp_split_f16": (c_int, [c_vp, c_int, c_int, c_int, c_vp, c_int, c_vp]),
    "tgp_planes_bytes": (c_i64, [c_i64, c_int]),
    "tgp_planes_split": (c_int, [c_vp, c_int, c_int, c_int, c_vp, c_int, c_vp, c_vp]),
    "tgp_planes_split_cols": (c_int, [c_vp, c_int, c_int, c_int, c_vp, c_int, c_int, c_vp, c_vp]),
    "tgp_planes_gather": (c_int, [c_vp, c_int, c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_int, c_vp, c_int, c_vp, c_vp]),
    "tgp_gemm_tn_workspace_floats": (c_i64, [c_i64, c_int, c_int]),
    "tgp_gemm_tn_f32": (c_int, [c_vp, c_int, c_vp, c_int, c_i64, c_int, c_int, c_vp, c_int, c_int, c_vp, c_vp]),
    "tgp_bw_workspace_floats": (c_i64, [c_i64, c_int]),
    "tgp_colsum": (c_int, [c_vp, c_int, c_i64, c_int, c_vp, c_int, c_vp, c_vp]),
    "tgp_bn_bwd": (c_int, [c_vp, c_int, c_vp, c_int, c_i64, c_int, c_vp, c_vp, c_f32, c_vp, c_vp, c_int, c_f32, c_vp,
                           c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "tgp_absmax_scale_from_bits": (c_int, [c_vp, c_int, c_f32, c_vp, c_vp]),
    "tgp_bn_bwd_absmax_words": (c_i64, [c_i64, c_int]),
    "tgp_bn_bwd_pooled": (c_int, [c_vp, c_int, c_vp, c_int, c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp, c_f32, c_vp, c_vp,
                                  c_int, c_f32, c_vp, c_vp, c_int, c_vp, c_vp, c_vp]),
    "tgp_colmax_arg": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp, c_f32, c_vp, c_vp, c_int, c_f32, c_vp, c_vp,
                               c_int, c_vp, c_int, c_vp]),
    "tgp_colsum_objects": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_vp, c_int, c_vp]),
    "tgp_colmax_bwd": (c_int, [c_vp, c_int, c_vp, c_int, c_int, c_int, c_int, c_vp, c_int, c_vp]),
    "tgp_transpose": (c_int, [c_vp, c_int, c_int, c_int, c_vp, c_int, c_vp]),
    "tgp_gconv_bwd_workspace_floats": (c_i64, [c_int, c_int, c_int]),
    "tgp_gconv_surface_bwd": (c_int, [c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp]),
    "tgp_gconv_hs_bwd": (c_int, [c_vp, c_vp, c_vp, c_int, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_int, c_vp,
                                 c_vp, c_vp]),
    "tgp_nbrmax_bwd": (c_int, [c_vp, c_int, c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_int, c_int, c_f32, c_vp, c_int, c_vp]),
    "tgp_iou3d_pairs": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_vp]),
    "tgp_rt_error_pairs": (c_int, [c_vp, c_vp, c_vp, c_int, c_vp, c_vp]),
    "tgp_absmax_scale": (c_int, [c_vp, c_int, c_i64, c_int, c_f32, c_vp, c_vp, c_vp]),
    "tgp_transpose_scaled": (c_int, [c_vp, c_int, c_int, c_int, c_vp, c_vp, c_int, c_vp]),
    "tgp_transpose_split_f16": (c_int, [c_vp, c_int, c_int, c_int, c_vp, c_vp, c_int, c_vp]),
    "tgp_sum_slabs": (c_int, [c_vp, c_int, c_i64, c_vp, c_vp, c_int, c_vp]),
    "tgp_pose_terms_fwd": (c_int, [c_vp] * 11 + [c_int, c_int, c_int, c_f32, c_vp, c_vp]),
    "tgp_pose_terms_bwd": (c_int, [c_vp] * 11 + [c_int, c_int, c_int, c_f32] + [c_vp] * 8 + [c_vp]),
    "tgp_sym_recon_workspace_floats": (c_i64, [c_int, c_int]),
    "tgp_sym_recon_fwd": (c_int, [c_vp] * 5 + [c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp]),
    "tgp_sym_recon_bwd": (c_int, [c_vp] * 5 + [c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp]),
    "tgp_rowl1_fwd": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_vp, c_vp, c_vp]),
    "tgp_rowl1_bwd": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_vp, c_vp]),
    "tgp_feat_consistency_fwd": (c_int, [c_vp, c_vp, c_int, c_int, c_vp, c_vp, c_vp]),
    "tgp_feat_consistency_bwd": (c_int, [c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_vp, c_vp, c_vp]),
    "tgp_pose_transform_fwd": (c_int, [c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_vp, c_vp]),
    "tgp_pose_transform_bwd": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "tgp_gather_rows_bwd": (c_int, [c_vp, c_int, c_vp, c_int, c_int, c_int, c_int, c_vp, c_int, c_vp]),
    "tgp_gemm_f32": (c_int, [ctypes.POINTER(GemmArgs), c_vp]),
    "tgp_colmax_decode": (c_int, [c_vp, c_int, c_int, c_int, c_vp, c_int, c_vp, c_vp]),
    "tgp_colmax": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp]),
    "tgp_sigmoid": (c_int, [c_vp, c_vp, c_i64, c_vp]),
    "tgp_head_post": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "tgp_add_mean": (c_int, [c_vp, c_vp, c_int, c_int, c_vp]),
    "tgp_bn_workspace_floats": (c_i64, [c_i64, c_int]),
    "tgp_bn_stats": (c_int, [c_vp, c_int, c_i64, c_int, c_vp, c_vp, c_vp, c_vp]),
    "tgp_bn_stats_running": (c_int, [c_vp, c_int, c_i64, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_f32, c_vp, c_vp]),
    "tgp_bn_apply": (c_int, [c_vp, c_int, c_i64, c_int, c_vp, c_vp, c_vp, c_vp, c_f32, c_int, c_f32, c_vp, c_vp, c_int, c_vp,
                             c_int, c_int, c_int, c_vp]),
    "tgp_dropout_apply": (c_int, [c_vp, c_vp, c_f32, c_i64, c_vp, c_vp]),
    "tgp_chamfer_fwd": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "tgp_chamfer_bwd": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "tgp_dcd_fwd": (c_int, [c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_f32, c_f32, c_int, c_vp, c_vp, c_vp, c_vp]),
    "tgp_dcd_bwd": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_f32, c_vp, c_vp, c_vp]),
    "tgp_emd_max_points": (c_int, []),
    "tgp_emd_workspace_bytes": (c_i64, [c_int, c_int]),
    "tgp_emd_fwd": (c_int, [c_vp, c_vp, c_int, c_int, c_f32, c_int, c_vp, c_vp, c_vp, c_vp]),
    "tgp_emd_bwd": (c_int, [c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_vp, c_vp]),
    "tgp_fps_max_points": (c_int, []),
    "tgp_fps": (c_int, [c_vp, c_int, c_vp, c_int, c_int, c_int, c_vp, c_int, c_vp, c_vp, c_vp, c_vp]),
    "tgp_render_max_faces": (c_int, []),
    "tgp_render_max_instances": (c_int, []),
    "tgp_render_workspace_bytes": (c_i64, [c_int, c_int, c_int]),
    "tgp_render_depth": (c_int, [ctypes.POINTER(RenderArgs), c_vp]),
    "tgp_generate_rt": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_vp, c_vp]),
    "tgp_canonicalize": (c_int, [c_vp] * 9 + [c_int, c_int, c_int, c_vp, c_vp, c_vp]),
    "tgp_heads_fused": (c_int, [ctypes.POINTER(HeadsFusedArgs), c_vp]),
    "tgp_conv_max_fused": (c_int, [ctypes.POINTER(ConvMaxFusedArgs), c_vp]),
    "tgp_heads_pack_w2": (c_int, [c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_vp]),
    "tgp_heads_w2_bytes": (c_i64, [c_int]),
    "tgp_dec_fused": (c_int, [ctypes.POINTER(DecFusedArgs), c_vp]),
    "tgp_hs_chain": (c_int, [ctypes.POINTER(HsChainArgs), c_vp]),
    "tgp_proj_planes": (c_int, [ctypes.POINTER(ProjPlanesArgs), c_vp]),
    "tgp_proj_pack_bytes": (c_i64, [c_int, c_int]),
    "tgp_proj_pack": (c_int, [c_vp, c_int, c_int, c_int, c_vp, c_vp]),
    "tgp_hs_chain_pack_bytes": (c_i64, [c_int, c_int, c_int]),
    "tgp_hs_chain_pack": (c_int, [c_vp, c_int, c_int, c_int, c_vp, c_int, c_int, c_vp, c_vp]),
    "tgp_dec_pack_bytes": (c_i64, []),
    "tgp_dec_pack": (c_int, [c_vp, c_vp, c_vp, c_int, c_vp, c_vp]),
    "tgp_dec_l1": (c_int, [ctypes.POINTER(DecL1Args), c_vp]),
    "tgp_ranger_plan": (c_int, [ctypes.POINTER(RangerTensor), c_int, ctypes.POINTER(c_i64)]),
    "tgp_ranger_step": (c_int, [ctypes.POINTER(RangerArgs), c_vp]),
    "tgp_augment_max_points": (c_int, []),
    "tgp_augment": (c_int, [ctypes.POINTER(AugmentArgs), c_vp]),
    "tgp_pd_workspace_bytes": (c_i64, []),
    "tgp_pd_max_points": (c_int, []),
    "tgp_persistence": (c_int, [ctypes.POINTER(PdArgs), c_vp]),
    "tgp_sort_by_parent": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "tgp_roi_cloud": (c_int, [c_vp] * 7 + [c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp]),
    "tgp_cloud_select": (c_int, [c_vp] * 5 + [c_int, c_int, c_int, c_vp, c_vp]),
    "tgp_pose_rotation_fwd": (c_int, [c_vp] * 6 + [c_int, c_vp, c_vp, c_vp]),
    "tgp_pose_rotation_bwd": (c_int, [c_vp, c_vp, c_int, c_vp, c_vp]),
    "tgp_rows_out": (c_int, [c_vp, c_int, c_i64, c_int, c_vp, c_int, c_vp, c_int, c_vp, c_int, c_vp, c_vp]),
    "tgp_rows_out_pred": (c_int, [c_vp, c_int, c_i64, c_int, c_vp, c_int, c_vp, c_int, c_vp, c_int, c_vp, c_vp, c_vp]),
    "tgp_pose_tail": (c_int, [c_vp] * 8 + [c_int] + [c_vp] * 8),
    "tgp_head_post_bwd": (c_int, [c_vp, c_vp, c_int, c_int, c_int] + [c_vp] * 10),
    "tgp_transpose_both": (c_int, [c_vp, c_int, c_int, c_int, c_vp, c_vp, c_int, c_vp]),
    "tgp_gemm_tn_split": (c_int, [c_vp, c_int, c_vp, c_int, c_int, c_int, c_int, c_vp, c_int, c_int, c_vp, c_vp]),
    "tgp_reverse_graph": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp]),
    "tgp_nbrmax_bwd_gather": (c_int, [c_vp, c_int, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_int, c_int, c_f32,
                                      c_vp, c_vp, c_int, c_vp]),
    "tgp_gconv_hs_bwd_gather": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int,
                                        c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_int, c_vp]),
    "tgp_gconv_hs_fwd_slots": (c_int, [c_vp, c_vp, c_vp, c_int, c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_int, c_vp, c_vp]),
    "tgp_child_lists": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp]),
    "tgp_segsum_rows": (c_int, [c_vp, c_int, c_int, c_vp, c_vp, c_int, c_vp, c_int, c_vp]),
    "tgp_roi_cloud_ex": (c_int, [c_vp] * 7 + [c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_f32, c_vp]),
    "tgp_cloud_select_ex": (c_int, [c_vp] * 5 + [c_int, c_int, c_int, c_vp, c_vp, c_vp]),
    "tgp_roi_band": (c_int, [c_vp] * 6 + [c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp]),
    "tgp_roi_cloud_defor": (c_int, [c_vp] * 7 + [c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_f32, c_vp, c_vp, c_int, c_vp]),
    "tgp_cloud_sample": (c_int, [c_vp] * 5 + [c_int, c_int, c_int, ctypes.c_uint64, c_vp, c_vp]),
    "tgp_gconv_dirgrad": (c_int, [c_vp, c_vp, c_vp, c_int, c_vp, c_vp, c_int, c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp]),
    "tgp_dirs_to_xyz": (c_int, [c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_vp, c_int, c_int, c_int, c_vp, c_int, c_vp]),
    "tgp_neighbor_dirs": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_vp, c_vp, c_vp]),
    "tgp_center_bwd": (c_int, [c_vp, c_vp, c_int, c_int, c_vp, c_vp]),
    "tgp_bn_eval_workspace_floats": (c_i64, [c_int]),
    "tgp_bn_eval_bwd": (c_int, [c_vp, c_int, c_vp, c_int, c_i64, c_int, c_vp, c_vp, c_f32, c_vp, c_vp, c_int, c_f32, c_vp, c_int, c_vp, c_vp,
                                c_vp, c_vp]),
    "tgp_bn_eval_bwd_pooled": (c_int, [c_vp, c_int, c_vp, c_int, c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp, c_f32, c_vp, c_vp, c_int,
                                       c_f32, c_vp, c_int, c_vp, c_vp, c_vp, c_vp]),
    "tgp_draw_words": (c_int, [c_vp, c_int, c_u64, c_u32, c_int, c_vp, c_vp]),
    "tgp_draw_band_subset": (c_int, [c_vp, c_vp, c_f64, c_vp, c_u64, c_int, c_int, c_vp, c_vp, c_int, c_vp]),
    "tgp_draw_alive": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp]),
    "tgp_draw_selection": (c_int, [c_vp, c_int, c_int, c_vp, c_u64, c_u32, c_int, c_int, c_int, c_vp, c_vp]),
    "tgp_draw_fill": (c_int, [c_vp, c_u64, c_int, c_int, c_vp, c_vp, c_f32, c_f32, c_vp, c_vp]),
    "tgp_gather_slots": (c_int, [ctypes.POINTER(GatherSlotsArgs), c_vp]),
    "tgp_mesh_area_cdf": (c_int, [c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_vp, c_vp]),
    "tgp_mesh_sample": (c_int, [ctypes.POINTER(MeshSampleArgs), c_vp]),
    "tgp_ball_cloud": (c_int, [c_vp] * 9 + [c_int] * 6 + [c_vp, c_vp, c_vp]),
    "tgp_ball_cloud_pts": (c_int, [c_vp] * 4 + [c_int] * 4 + [c_vp, c_vp, c_vp]),
    "tgp_ball_select": (c_int, [c_vp] * 7 + [c_int] * 6 + [c_vp, c_vp, c_vp]),
    "tgp_ball_sample": (c_int, [c_vp] * 6 + [c_int] * 6 + [c_u64, c_vp, c_vp, c_vp]),
}

ABI_VERSION = 8
_lib = None


class TgpError(RuntimeError):
    pass


def lib():
    """Load the shared library once; raise loudly if it is not there."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise TgpError(
                "tgpose_amd: %s not found. Build it with `python -m tgpose_amd.build` (hipcc, gfx950). "
                "There is no CPU/torch fallback for the HIP path." % LIB_PATH)
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the symbol is missing
            fn.restype = res
            fn.argtypes = args
        if handle.tgp_version() != ABI_VERSION:
            raise TgpError("tgpose_amd: ABI version mismatch (%d != %d)" % (handle.tgp_version(), ABI_VERSION))
        if os.environ.get("TGP_TRACE", "0") != "0":
            # diagnosis: every entry point announces itself on stderr before it launches (with HIP_LAUNCH_BLOCKING=1 the last
            # name printed is the launch that faulted)
            class _Traced(object):
                def __init__(self, h):
                    self._h = h

                def __getattr__(self, name):
                    fn = getattr(self._h, name)

                    def call(*a):
                        sys.stderr.write("tgp: %s\n" % name)
                        sys.stderr.flush()
                        return fn(*a)
                    return call
            handle = _Traced(handle)
        _lib = handle
    return _lib


_ERR = {-1: "TGP_EINVAL (bad pointer / size / stride / alignment)", -2: "TGP_EUNSUPPORTED (shape not supported)"}


def check(rc, what):
    if rc != 0:
        raise TgpError("%s failed: %s" % (what, _ERR.get(rc, "hipError_t %d" % rc)))
