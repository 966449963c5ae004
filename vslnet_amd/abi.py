"""The foreign interface of libvslnet_hip.so (include/vslnet_hip.h), stated once: the ctypes mirrors of its structs, ONE table of its prototypes
(`PROTOTYPES`: what load_library binds, and what ABI_SYMBOLS is derived from), ONE table of the features an older build may lack (`FEATURES`: the
symbols each needs and the text of its refusal), the loader, and the tuples the engine's calls return.  A new entry point is a mirror (when it has a
struct), a line in PROTOTYPES and, when older builds lack it, a line in FEATURES.  tests/test_abi_layout.py checks every mirror's layout and every
prototype against the header."""
import ctypes as C
import os
from collections import namedtuple

from . import build as _build

_LIB = None
ABI_VERSION = 9                                     # include/vslnet_hip.h: VSL_ABI_VERSION


class VslError(RuntimeError):
    pass


# ---- the structs ------------------------------------------------------------------------------------------------
class vsl_config(C.Structure):
    _fields_ = [('dim', C.c_int32), ('num_heads', C.c_int32), ('max_pos_len', C.c_int32),
                ('video_feature_dim', C.c_int32), ('word_dim', C.c_int32), ('char_dim', C.c_int32),
                ('word_size', C.c_int32), ('char_size', C.c_int32), ('predictor', C.c_int32), ('drop_rate', C.c_float),
                ('word_table', C.c_int32)]


class vsl_io(C.Structure):
    _fields_ = [('B', C.c_int32), ('T', C.c_int32), ('Lq', C.c_int32), ('Lc', C.c_int32),
                ('params', C.c_void_p), ('pad_vec', C.c_void_p), ('glove_vec', C.c_void_p),
                ('word_ids', C.c_void_p), ('char_ids', C.c_void_p), ('video_features', C.c_void_p),
                ('v_mask', C.c_void_p), ('q_mask', C.c_void_p),
                ('h_score', C.c_void_p), ('start_logits', C.c_void_p), ('end_logits', C.c_void_p),
                ('workspace', C.c_void_p), ('training', C.c_int32), ('seed', C.c_uint64),
                ('d_h_score', C.c_void_p), ('d_start_logits', C.c_void_p), ('d_end_logits', C.c_void_p),
                ('grads', C.c_void_p), ('sample_offset', C.c_int32), ('video_features_bf16', C.c_void_p),
                ('early_grads_event', C.c_void_p),
                ('fused_step', C.c_void_p),        # (NULL unless Engine.backward(fused_step=...): an older build loaded for an A/B run reads zeros here)
                ('fused_loss', C.c_void_p),        # (NULL unless the last loss() was lazy=True)
                ('inference', C.c_int32)]          # (1: Engine.forward(inference=True); an older build loaded for an A/B run never reads it)


class vsl_encode_io(C.Structure):
    _fields_ = [('N', C.c_int32), ('T', C.c_int32), ('params', C.c_void_p), ('video_features', C.c_void_p), ('video_features_bf16', C.c_void_p),
                ('v_mask', C.c_void_p), ('video_encoding', C.c_void_p), ('workspace', C.c_void_p)]


class vsl_localize_io(C.Structure):
    _fields_ = [('B', C.c_int32), ('T', C.c_int32), ('Lq', C.c_int32), ('Lc', C.c_int32), ('N', C.c_int32),
                ('params', C.c_void_p), ('pad_vec', C.c_void_p), ('glove_vec', C.c_void_p),
                ('word_ids', C.c_void_p), ('char_ids', C.c_void_p), ('q_mask', C.c_void_p),
                ('video_encoding', C.c_void_p), ('v_mask', C.c_void_p), ('video_index', C.c_void_p),
                ('h_score', C.c_void_p), ('start_logits', C.c_void_p), ('end_logits', C.c_void_p), ('workspace', C.c_void_p)]


class vsl_shared_io(C.Structure):
    _fields_ = [('N', C.c_int32), ('video_index', C.c_void_p), ('video_v_mask', C.c_void_p)]


class vsl_encode_query_io(C.Structure):
    _fields_ = [('Q', C.c_int32), ('Lq', C.c_int32), ('Lc', C.c_int32), ('params', C.c_void_p), ('pad_vec', C.c_void_p), ('glove_vec', C.c_void_p),
                ('word_ids', C.c_void_p), ('char_ids', C.c_void_p), ('q_mask', C.c_void_p), ('query_encoding', C.c_void_p), ('workspace', C.c_void_p)]


class vsl_pairs_io(C.Structure):
    _fields_ = [('B', C.c_int32), ('T', C.c_int32), ('Lq', C.c_int32), ('N', C.c_int32), ('Q', C.c_int32),
                ('params', C.c_void_p), ('video_encoding', C.c_void_p), ('v_mask', C.c_void_p), ('query_encoding', C.c_void_p), ('q_mask', C.c_void_p),
                ('video_index', C.c_void_p), ('query_index', C.c_void_p),
                ('h_score', C.c_void_p), ('start_logits', C.c_void_p), ('end_logits', C.c_void_p), ('workspace', C.c_void_p)]


class vsl_highlight_io(C.Structure):
    _fields_ = [('pairs', vsl_pairs_io), ('relevance', C.c_int32), ('ld', C.c_int32), ('out', C.c_void_p)]


class vsl_select_io(C.Structure):
    _fields_ = [('G', C.c_int32), ('N', C.c_int32), ('ld', C.c_int32), ('M', C.c_int32), ('key', C.c_void_p), ('out_index', C.c_void_p),
                ('out_key', C.c_void_p), ('out_count', C.c_void_p)]


class vsl_loss_io(C.Structure):
    _fields_ = [('start_labels', C.c_void_p), ('end_labels', C.c_void_p), ('h_labels', C.c_void_p),
                ('w_loc', C.c_float), ('w_highlight', C.c_float), ('inv_batch', C.c_float), ('mask_sum', C.c_float),
                ('losses', C.c_void_p), ('d_h_score', C.c_void_p), ('d_start_logits', C.c_void_p),
                ('d_end_logits', C.c_void_p)]


class vsl_group_loss_io(C.Structure):
    _fields_ = [('B', C.c_int32), ('T', C.c_int32), ('G', C.c_int32),
                ('h_score', C.c_void_p), ('start_logits', C.c_void_p), ('end_logits', C.c_void_p), ('v_mask', C.c_void_p),
                ('start_labels', C.c_void_p), ('end_labels', C.c_void_p), ('h_labels', C.c_void_p),
                ('group_start', C.c_void_p), ('positive', C.c_void_p),
                ('w_loc', C.c_float), ('w_highlight', C.c_float), ('w_rank', C.c_float), ('inv_pos', C.c_float), ('inv_groups', C.c_float),
                ('mask_sum', C.c_float), ('inv_temperature', C.c_float), ('relevance', C.c_int32),
                ('losses', C.c_void_p), ('hits', C.c_void_p), ('pair_relevance', C.c_void_p),
                ('d_h_score', C.c_void_p), ('d_start_logits', C.c_void_p), ('d_end_logits', C.c_void_p), ('scratch', C.c_void_p)]


class vsl_adamw(C.Structure):
    _fields_ = [('lr', C.c_float), ('beta1', C.c_float), ('beta2', C.c_float), ('eps', C.c_float), ('weight_decay', C.c_float),
                ('clip_norm', C.c_float), ('step', C.c_int32), ('hf_order', C.c_int32), ('norm_from_backward', C.c_int32)]


class vsl_fused_step(C.Structure):
    _fields_ = [('params', C.c_void_p), ('exp_avg', C.c_void_p), ('exp_avg_sq', C.c_void_p), ('hp', vsl_adamw), ('grad_norm_out', C.c_void_p)]


class vsl_topk_io(C.Structure):
    _fields_ = [('start_logits', C.c_void_p), ('end_logits', C.c_void_p), ('valid_len', C.c_void_p),
                ('B', C.c_int), ('T', C.c_int), ('K', C.c_int), ('nms_iou', C.c_float), ('max_span', C.c_int),
                ('start_index', C.c_void_p), ('end_index', C.c_void_p), ('score', C.c_void_p), ('prob', C.c_void_p), ('count', C.c_void_p)]


class vsl_merge_io(C.Structure):
    _fields_ = [('B', C.c_int), ('K', C.c_int), ('G', C.c_int), ('K_out', C.c_int),
                ('start', C.c_void_p), ('end', C.c_void_p), ('score', C.c_void_p), ('key', C.c_void_p), ('count', C.c_void_p),
                ('group_index', C.c_void_p), ('tag', C.c_void_p), ('tag_per_slot', C.c_int32),
                ('out_tag', C.c_void_p), ('out_list', C.c_void_p), ('out_start', C.c_void_p), ('out_end', C.c_void_p),
                ('out_score', C.c_void_p), ('out_key', C.c_void_p), ('out_count', C.c_void_p)]


class vsl_encode_windows_io(C.Structure):
    _fields_ = [('rows', C.c_int32), ('N', C.c_int32), ('T', C.c_int32), ('params', C.c_void_p), ('video_features', C.c_void_p),
                ('video_features_bf16', C.c_void_p), ('window_row', C.c_void_p), ('window_len', C.c_void_p), ('video_encoding', C.c_void_p),
                ('v_mask', C.c_void_p), ('workspace', C.c_void_p)]


class vsl_merge_windows_io(C.Structure):
    _fields_ = [('B', C.c_int), ('K', C.c_int), ('G', C.c_int), ('K_out', C.c_int), ('nms_iou', C.c_float),
                ('start', C.c_void_p), ('end', C.c_void_p), ('score', C.c_void_p), ('key', C.c_void_p), ('count', C.c_void_p),
                ('group_index', C.c_void_p), ('offset', C.c_void_p),
                ('out_list', C.c_void_p), ('out_start', C.c_void_p), ('out_end', C.c_void_p), ('out_score', C.c_void_p), ('out_key', C.c_void_p),
                ('out_count', C.c_void_p)]


# ---- what the engine's calls return -----------------------------------------------------------------------------
# what Engine.select_topm / VSLNet.rank_videos return, per group (query): (G, m) int32 video (the index), fp32 relevance (the key), (G,) int32 count =
# min(m, N); ranked: relevance descending, ties by the smaller index; slots from count[g] on hold -1, 0
VideoRanks = namedtuple('VideoRanks', 'video relevance count')
RELEVANCE = {'max': 0, 'mean': 1}                   # vsl_highlight_io.relevance
TOPM_MAX_M = 1024                                   # vsl_select_topm: the largest M
# what Engine.extract_topk returns: (B, K) int64 start / end, (B, K) fp32 score (the logit sum) and prob (None without want_prob), (B,) int32 count;
# slots from count[b] on hold -1, -1, -inf, 0
TopkSpans = namedtuple('TopkSpans', 'start end score prob count')
# what Engine.merge_topk returns, per group: (G, k_out) int32 tag and list (the input list a slot came from), int64 start / end, fp32 score and prob
# (the ranking key), (G,) int32 count; slots from count[g] on hold -1, -1, -1, -1, -inf, 0
CorpusMoments = namedtuple('CorpusMoments', 'tag list start end score prob count')
# what Engine.merge_windows returns, per group: (G, k_out) int32 list (the input list a slot came from), int64 start / end in the video's own clips,
# fp32 score and prob (the ranking key), (G,) int32 count; slots from count[g] on hold -1, -1, -1, -inf, 0
WindowMoments = namedtuple('WindowMoments', 'list start end score prob count')
# what VSLNet.localize_long returns, per (video, query) pair: the same with `window` (the row of the WindowEncoding a moment came from) in place of `list`
LongMoments = namedtuple('LongMoments', 'window start end score prob count')


# ---- the prototypes: symbol -> (argtypes, restype) ----------------------------------------------------------------
_H = C.c_void_p                                     # a vsl_handle, a device pointer, a hipStream_t
_I, _S = C.c_int, C.c_char_p
_I32P, _I64P, _F64P = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)


def _enqueues(*structs):
    """int f(vsl_handle, const <struct>*..., void* hip_stream)"""
    return [_H] + [C.POINTER(s) for s in structs] + [_H], _I


def _floats(n):
    """int f(vsl_handle, <n ints: the shape>, int64_t* out)"""
    return [_H] + [_I] * n + [_I64P], _I


PROTOTYPES = {
    'vsl_abi_version': ([], _I),
    'vsl_last_error': ([], _S),
    'vsl_create': ([C.POINTER(vsl_config), C.POINTER(_H)], _I),
    'vsl_destroy': ([_H], _I),
    'vsl_param_count': ([_H], _I),
    'vsl_param_info': ([_H, _I, _S, _I, _I64P, _I64P, _I32P, _I64P], _I),
    'vsl_param_floats': ([_H], C.c_int64),
    'vsl_workspace_floats': _floats(4),
    'vsl_inference_workspace_floats': _floats(4),
    'vsl_forward': _enqueues(vsl_io),
    'vsl_encode_workspace_floats': _floats(2),
    'vsl_encode_video': _enqueues(vsl_encode_io),
    'vsl_localize_workspace_floats': _floats(4),
    'vsl_localize': _enqueues(vsl_localize_io),
    'vsl_encode_query_workspace_floats': _floats(3),
    'vsl_encode_query': _enqueues(vsl_encode_query_io),
    'vsl_pairs_workspace_floats': _floats(3),
    'vsl_localize_pairs': _enqueues(vsl_pairs_io),
    'vsl_highlight_pairs': _enqueues(vsl_highlight_io),
    'vsl_select_topm': _enqueues(vsl_select_io),
    'vsl_shared_workspace_floats': _floats(5),
    'vsl_forward_shared': _enqueues(vsl_io, vsl_shared_io),
    'vsl_backward_shared': _enqueues(vsl_io, vsl_shared_io),
    'vsl_shared_workspace_offset': ([_H, _I, _I, _I, _I, _I, _S], C.c_int64),
    'vsl_loss': _enqueues(vsl_io, vsl_loss_io),
    'vsl_group_loss_scratch_floats': ([_I, _I, _I64P], _I),
    'vsl_group_loss': _enqueues(vsl_group_loss_io),
    'vsl_backward': _enqueues(vsl_io),
    'vsl_backward_accumulate': _enqueues(vsl_io, vsl_shared_io),
    'vsl_input_grads': ([_H, C.POINTER(vsl_io), C.POINTER(vsl_shared_io), _H, _H], _I),
    'vsl_early_grad_offset': ([_H], C.c_int64),
    'vsl_debug_rnn_launches': ([C.c_uint64], C.c_uint64),
    'vsl_extract_index': ([_H, _H, _H, _I, _I, _H, _H, _H], _I),
    'vsl_extract_topk': _enqueues(vsl_topk_io),
    'vsl_merge_topk': _enqueues(vsl_merge_io),
    'vsl_encode_windows_workspace_floats': _floats(3),
    'vsl_encode_windows': _enqueues(vsl_encode_windows_io),
    'vsl_merge_windows': _enqueues(vsl_merge_windows_io),
    'vsl_adamw_step': ([_H, _H, _H, _H, _H, C.POINTER(vsl_adamw), _H, _H], _I),
    'vsl_workspace_offset': ([_H, _I, _I, _I, _I, _S], C.c_int64),
    'vsl_profile_select': ([_H, _S], _I),
    'vsl_profile_read': ([_H, _I, _S, _I, _F64P, _I32P], _I),
    'vsl_profile_launch': ([_H, _I, _S, _I, _I32P, _F64P, _F64P, _F64P, _I32P, _I32P], _I),
}
ABI_SYMBOLS = list(PROTOTYPES)

# ---- what an older build (loaded through VSLNET_HIP_LIB for an A/B run) may lack: Engine.has_<flag> -> (the symbols it needs, its refusal) ----------
FEATURES = {
    # the forward-only plan; without it forward(inference=True) raises and the module's no_grad path keeps the saved path
    'inference': (('vsl_inference_workspace_floats',), 'the loaded library has no inference mode (vsl_inference_workspace_floats is missing)'),
    # one encoding per video, many queries against it
    'shared_video': (('vsl_encode_video', 'vsl_localize'), 'the loaded library has no shared-video entry points (vsl_encode_video / vsl_localize are missing)'),
    # a training step over N videos and B queries
    'shared_train': (('vsl_forward_shared', 'vsl_backward_shared'),
                     'the loaded library has no shared-encoding training step (vsl_forward_shared / vsl_backward_shared are missing)'),
    # a backward that adds to the gradient bucket (one optimizer step over K micro-batches)
    'grad_accumulation': (('vsl_backward_accumulate',),
                          'backward(accumulate=True): the loaded library has no gradient accumulation (vsl_backward_accumulate is missing)'),
    # the K best spans per sample with temporal NMS
    'topk': (('vsl_extract_topk',), 'the loaded library has no top-k span extraction (vsl_extract_topk is missing)'),
    # the gradient with respect to the video features, one launch behind a backward
    'input_grads': (('vsl_input_grads',), 'the loaded library has no input gradients (vsl_input_grads is missing)'),
    # the k_out best moments of every group of top-K lists (a search over several videos)
    'merge_topk': (('vsl_merge_topk',), 'the loaded library has no cross-list merge (vsl_merge_topk is missing)'),
    # the query half of the inference forward, once per query, and vsl_localize_pairs, which reads it: both or neither
    'query_encoding': (('vsl_encode_query', 'vsl_encode_query_workspace_floats', 'vsl_localize_pairs', 'vsl_pairs_workspace_floats'),
                       'the loaded library has no query encodings (vsl_encode_query / vsl_localize_pairs are missing)'),
    # sliding windows over a video of any length
    'windows': (('vsl_encode_windows', 'vsl_encode_windows_workspace_floats', 'vsl_merge_windows'),
                'the loaded library has no sliding windows (vsl_encode_windows / vsl_merge_windows are missing)'),
    # rank the videos of a corpus by highlight score (without it VSLNet.retrieve serves prefilter=0 only)
    'video_ranking': (('vsl_highlight_pairs', 'vsl_select_topm'), 'the loaded library cannot rank videos (vsl_highlight_pairs / vsl_select_topm are missing)'),
    # the span / highlight losses over groups of pair rows + the video ranking term
    'group_loss': (('vsl_group_loss', 'vsl_group_loss_scratch_floats'),
                   'the loaded library has no video ranking loss (vsl_group_loss / vsl_group_loss_scratch_floats are missing)'),
}


def load_library():
    """dlopen libvslnet_hip.so (building it in-tree with hipcc when stale/missing).  Raises if that fails."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = os.environ.get('VSLNET_HIP_LIB')        # A/B runs: an alternative build of the same ABI
    explicit = bool(path)
    if not path:
        path = _build.LIB
        if not os.path.exists(path) or _build._stale():
            # several ranks of one node may get here together (torch.distributed.run): one builds, the others wait for it
            import fcntl
            os.makedirs(_build.LIBDIR, exist_ok=True)
            with open(os.path.join(_build.LIBDIR, '.build.lock'), 'w') as lock:
                fcntl.flock(lock, fcntl.LOCK_EX)
                try:
                    if not os.path.exists(path) or _build._stale():
                        path = _build.build()
                finally:
                    fcntl.flock(lock, fcntl.LOCK_UN)
    lib = C.CDLL(path)
    # an A/B baseline built from an older revision (tools/build_base.py) may predate the check: new vsl_io fields are appended, so an older
    # library simply does not read them
    if not explicit and (not hasattr(lib, 'vsl_abi_version') or lib.vsl_abi_version() != ABI_VERSION):
        raise VslError('%s implements another ABI version than this binding (%d): rebuild it (python -m vslnet_amd.build --force)' % (path, ABI_VERSION))
    for name, (argtypes, restype) in PROTOTYPES.items():
        if hasattr(lib, name):                      # (a symbol an older build lacks: the engine's has_* flags refuse what needs it, by name)
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = argtypes, restype
    _LIB = lib
    return lib
