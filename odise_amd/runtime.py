"""Host-side runtime over the C ABI: one Context per process/GPU, device buffers, op wrappers.

One process per GPU (SURVEY.md §8b "threading / process model"): the Context binds to `cuda:<LOCAL_RANK>`,
owns one HIP stream, and is not re-entrant.  numpy arrays are the host-side currency (fp16/fp32); torch is
only used by callers for CPU tensors and `torch.distributed`.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._lib import ACT_NONE, F16, F32, U8, AttnDesc, ConvDesc, GemmDesc, check

_NP = {F16: np.float16, F32: np.float32}


class DeviceArray:
    """A hipMalloc'ed buffer with shape/dtype metadata (dtype is a numpy dtype)."""

    def __init__(self, ctx: "Context", shape: Sequence[int], dtype):
        self.ctx = ctx
        self.shape = tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        p = C.c_void_p()
        check(ctx.lib.odise_hip_malloc(ctx.h, C.c_size_t(max(self.nbytes, 16)), C.byref(p)), "malloc")
        self.ptr = p.value
        self._owned = True

    def view(self, shape, dtype=None, offset_bytes: int = 0) -> "DeviceArray":
        """Non-owning array over (a slice of) this buffer; keeps the owner alive."""
        v = DeviceArray.__new__(DeviceArray)
        v.ctx = self.ctx
        v.shape = tuple(int(x) for x in shape)
        v.dtype = np.dtype(dtype if dtype is not None else self.dtype)
        v.nbytes = int(np.prod(v.shape, dtype=np.int64)) * v.dtype.itemsize
        assert offset_bytes >= 0 and offset_bytes + v.nbytes <= self.nbytes, "view out of range"
        v.ptr = self.ptr + offset_bytes
        v._owned = False
        v._base = self
        return v

    def free(self):
        if self._owned and self.ptr and self.ctx.h:
            self.ctx.lib.odise_hip_free(self.ctx.h, C.c_void_p(self.ptr))
        self.ptr = None
        self._owned = False

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def numpy(self) -> np.ndarray:
        out = np.empty(self.shape, dtype=self.dtype)
        check(self.ctx.lib.odise_hip_memcpy_d2h(self.ctx.h, out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr),
                                                C.c_size_t(self.nbytes)), "memcpy_d2h")
        return out

    def copy_from(self, host: np.ndarray) -> "DeviceArray":
        host = np.ascontiguousarray(host, dtype=self.dtype)
        assert host.shape == self.shape, (host.shape, self.shape)
        check(self.ctx.lib.odise_hip_memcpy_h2d(self.ctx.h, C.c_void_p(self.ptr), host.ctypes.data_as(C.c_void_p),
                                                C.c_size_t(self.nbytes)), "memcpy_h2d")
        return self


class InstanceAccumulateError(RuntimeError):
    """`Context.instance_accumulate` raised a flag (instance_eval.ACCUM_FLAG_NAMES); .precision / .recall are what the device wrote."""

    def __init__(self, flags: int, precision: np.ndarray, recall: np.ndarray):
        from .instance_eval import accumulate_flag_names
        super().__init__("instance accumulate: malformed input(s): " + "; ".join(accumulate_flag_names(flags)))
        self.flags, self.precision, self.recall = flags, precision, recall


def _p(a: Optional[DeviceArray]):
    return C.c_void_p(a.ptr) if a is not None else C.c_void_p(None)


def _ptr(a):
    return a.ptr if isinstance(a, DeviceArray) else a


def _mask_dtype(masks: DeviceArray, what: str) -> int:
    """ODISE_F32 / ODISE_U8 of dense masks (float32, or uint8 / bool; nonzero = 1)."""
    dt = {np.dtype(np.float32): F32, np.dtype(np.uint8): U8, np.dtype(np.bool_): U8}.get(np.dtype(masks.dtype))
    if dt is None:
        raise ValueError(f"{what}: masks of dtype {masks.dtype} (float32, uint8 or bool)")
    return dt


def _fill_inst_source(d, what: str, hw, topk: int, table_row, scores_row, masks: Optional[DeviceArray], b: int, pad_hw, img_hw) -> None:
    """The detection fields that InstEvalDesc, InstDrawDesc and InstTrackDesc share: dense `masks` [topk, h, w], or the selection
    table_row / scores_row (DeviceArray or pointer) of image b of the last head forward."""
    d.h, d.w, d.topk = int(hw[0]), int(hw[1]), int(topk)
    if masks is not None:
        assert tuple(masks.shape) == (d.topk, d.h, d.w), (masks.shape, topk, hw)
        d.masks, d.dtype = masks.ptr, _mask_dtype(masks, what)
    d.b, d.pad_h, d.pad_w, d.img_h, d.img_w = int(b), int(pad_hw[0]), int(pad_hw[1]), int(img_hw[0]), int(img_hw[1])
    d.inst_table, d.inst_scores = _ptr(table_row), _ptr(scores_row)


def _boundary_task(boundary):
    """InstBoundaryTask of (rows, n_rows) or (rows, n_rows, radius); device arrays or pointers."""
    from ._lib import InstBoundaryTask
    t = InstBoundaryTask()
    t.rows, t.n_rows, t.radius = _ptr(boundary[0]), _ptr(boundary[1]), int(boundary[2]) if len(boundary) > 2 else 0
    return t


def _labels_or_scores(pred: DeviceArray, K: Optional[int]):
    """pred = labels int32 [H,W] (needs K) or sem_seg float32 [K,H,W] -> (labels, sem, K, H, W), one of the first two None."""
    if pred.dtype == np.float32:
        assert len(pred.shape) == 3 and (K is None or int(K) == pred.shape[0]), (pred.shape, K)
        K, H, W = pred.shape
        return None, pred, int(K), H, W
    assert pred.dtype == np.int32 and len(pred.shape) == 2 and K is not None, (pred.dtype, pred.shape, K)
    H, W = pred.shape
    return pred, None, int(K), H, W


def _fill_track_dumps(d, live, n_live, iou, live_cap, iou_cap) -> None:
    """The optional dumps that TrackDesc, InstTrackDesc and BoxTrackDesc share: live [cap] records of video.TRACK_ROW_DTYPE with n_live
    int32 [1], iou float64 [cap, MAX_SEGMENTS]; live_cap / iou_cap: fewer rows than the arrays hold."""
    from ._lib import MAX_SEGMENTS
    from .video import TRACK_ROW_DTYPE
    if live is not None:
        assert live.dtype == TRACK_ROW_DTYPE and (n_live is None or n_live.dtype == np.int32)
        d.live, d.live_cap = live.ptr, live.shape[0] if live_cap is None else int(live_cap)
        assert d.live_cap <= live.shape[0]
    if n_live is not None:
        d.n_live = n_live.ptr
    if iou is not None:
        assert iou.dtype == np.float64 and len(iou.shape) == 2 and iou.shape[1] == MAX_SEGMENTS, (iou.dtype, iou.shape)
        d.iou, d.iou_cap = iou.ptr, iou.shape[0] if iou_cap is None else int(iou_cap)
        assert d.iou_cap <= iou.shape[0]


def _inst_eval_desc(what: str, *, out_hw, table_row, scores_row, topk, gt: dict, num_categories, image, rows, n_rows, flags, masks, b, pad_hw,
                    img_hw, iou_thresholds):
    """-> (InstEvalDesc, the host threshold array it points to) of the arguments that `instance_eval` and `instance_eval_bbox` share."""
    from ._lib import InstEvalDesc
    from .instance_eval import IOU_THRS
    thr = np.ascontiguousarray(IOU_THRS if iou_thresholds is None else iou_thresholds, np.float64)
    assert thr.shape == (10,), thr.shape
    d = InstEvalDesc()
    _fill_inst_source(d, what, out_hw, topk, table_row, scores_row, masks, b, pad_hw, img_hw)
    d.gt_runs, d.gt_offsets, d.gt_rows, d.n_gt = gt["runs"].ptr, gt["offsets"].ptr, gt["rows"].ptr, int(gt["n_gt"])
    d.num_categories, d.image, d.iou_thresholds = int(num_categories), int(image), thr.ctypes.data
    d.rows, d.n_rows, d.flags = _ptr(rows), _ptr(n_rows), _ptr(flags)
    return d, thr


def _inst_poly_gt(gt: dict):
    """byref(InstPolyGt) of a ground truth that carries polygons (`instance_gt_to_device`), else None."""
    from ._lib import InstPolyGt
    if "gt_polys" not in gt:
        return None
    p = InstPolyGt()
    p.xy, p.poly_offsets, p.gt_polys, p.n_poly = gt["xy"].ptr, gt["poly_offsets"].ptr, gt["gt_polys"].ptr, int(gt["n_poly"])
    return C.byref(p)


class Context:
    def __init__(self, device: int = 0):
        self.lib = _lib.load()
        h = C.c_void_p()
        check(self.lib.odise_hip_create(C.c_int(device), C.byref(h)), "create")
        self.h = h
        self.device = device
        # A context holds ONE model (the library's weight store is per context): the host wrapper that loaded weights last registers itself
        # here, so long-lived holders of a wrapper (test fixtures, servers swapping models) can tell whether theirs is still the resident one.
        self.model_owner = None

    def close(self):
        if self.h:
            self.lib.odise_hip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- memory -----------------------------------------------------------------------------
    def empty(self, shape, dtype=np.float16) -> DeviceArray:
        return DeviceArray(self, shape, dtype)

    def zeros(self, shape, dtype=np.float16) -> DeviceArray:
        a = DeviceArray(self, shape, dtype)
        check(self.lib.odise_hip_memset(self.h, C.c_void_p(a.ptr), 0, C.c_size_t(a.nbytes)), "memset")
        return a

    def to_device(self, host, dtype=None) -> DeviceArray:
        if hasattr(host, "detach"):  # torch CPU tensor
            host = host.detach().cpu().numpy()
        host = np.ascontiguousarray(host, dtype=dtype if dtype is not None else host.dtype)
        return DeviceArray(self, host.shape, host.dtype).copy_from(host)

    def sync(self):
        check(self.lib.odise_hip_sync(self.h), "sync")

    # ---- per-context execution options (include/odise_hip.h ODISE_OPT_*) ---------------------
    OPT_CLIP_LN_FOLD, OPT_VAE_CHUNK_BYTES, OPT_ATTN_KV_RESIDENT, OPT_PREFETCH_CU_EIGHTHS, OPT_PREFETCH_START, OPT_MASKCLIP_PASSES = 1, 2, 3, 4, 5, 6

    def set_option(self, option: int, value: int) -> None:
        check(self.lib.odise_hip_set_option(self.h, option, value), "set_option")

    def get_option(self, option: int) -> int:
        v = C.c_int64()
        check(self.lib.odise_hip_get_option(self.h, option, C.byref(v)), "get_option")
        return int(v.value)

    def stage_timeline(self, on: bool = True) -> None:
        check(self.lib.odise_hip_stage_timeline(self.h, 1 if on else 0), "stage_timeline")

    def stage_timeline_read(self):
        """[(name, gpu_ms, host_ms)] of the stage boundaries since stage_timeline(True), relative to the first."""
        cap = 8192
        names = C.create_string_buffer(1 << 20)
        g = (C.c_float * cap)()
        h = (C.c_double * cap)()
        n = C.c_int()
        check(self.lib.odise_hip_stage_timeline_read(self.h, names, len(names), g, h, cap, C.byref(n)), "stage_timeline_read")
        nm = names.value.decode().split("\n")
        return [(nm[i], float(g[i]), float(h[i])) for i in range(min(n.value, cap))]

    def launch_log(self, on: bool = True) -> None:
        check(self.lib.odise_hip_launch_log(self.h, 1 if on else 0), "launch_log")

    def launch_log_read(self) -> np.ndarray:
        """[n, 6] int32 records (conv, M, N, K, tile id, split-K) of the GEMM / conv launches since launch_log(True)."""
        n = C.c_int()
        check(self.lib.odise_hip_launch_log_read(self.h, None, 0, C.byref(n)), "launch_log_read")
        out = np.zeros((max(n.value, 1), 6), np.int32)
        check(self.lib.odise_hip_launch_log_read(self.h, out.ctypes.data_as(C.c_void_p), n.value, C.byref(n)), "launch_log_read")
        return out[: n.value]

    # ---- launch probe: per-launch durations of one GEMM / conv shape as it runs inside a step ------
    def probe_arm(self, conv: bool, M: int, N: int, K: int, max_launches: int = 256) -> None:
        check(self.lib.odise_hip_probe_arm(self.h, 1 if conv else 0, M, N, K, max_launches), "probe_arm")

    def probe_read(self, cap: int = 4096) -> np.ndarray:
        us = np.zeros(cap, np.float32)
        n = C.c_int()
        check(self.lib.odise_hip_probe_read(self.h, us.ctypes.data_as(C.c_void_p), cap, C.byref(n)), "probe_read")
        return us[: min(cap, n.value)].copy()

    def timer_start(self):
        check(self.lib.odise_hip_timer_start(self.h), "timer_start")

    def timer_stop(self) -> float:
        ms = C.c_float()
        check(self.lib.odise_hip_timer_stop(self.h, C.byref(ms)), "timer_stop")
        return float(ms.value)

    def device_info(self):
        buf = C.create_string_buffer(256)
        cu = C.c_int()
        mem = C.c_size_t()
        check(self.lib.odise_hip_device_info(self.h, buf, 256, C.byref(cu), C.byref(mem)), "device_info")
        return buf.value.decode(), cu.value, mem.value

    # ---- ops --------------------------------------------------------------------------------
    def ms_deform_attn_forward(self, value: DeviceArray, spatial_shapes, level_start_index, sampling_loc: DeviceArray,
                               attn_weight: DeviceArray, im2col_step: int = 128) -> DeviceArray:
        """MSDA.ms_deform_attn_forward (ms_deform_attn.h:25-44): value [B,S,M,D] -> [B,Lq,M*D]."""
        B, S, M, D = value.shape
        _, Lq, M2, L, P, two = sampling_loc.shape
        assert M2 == M and two == 2 and attn_weight.shape == (B, Lq, M, L, P)
        ss = np.ascontiguousarray(np.asarray(spatial_shapes, dtype=np.int64).reshape(L, 2))
        ls = np.ascontiguousarray(np.asarray(level_start_index, dtype=np.int64).reshape(L))
        assert sampling_loc.dtype == np.float32 and attn_weight.dtype == np.float32
        dt = F32 if value.dtype == np.float32 else F16
        out = self.empty((B, Lq, M * D), value.dtype)
        check(self.lib.odise_hip_ms_deform_attn_forward(
            self.h, _p(value), ss.ctypes.data_as(C.POINTER(C.c_int64)), ls.ctypes.data_as(C.POINTER(C.c_int64)),
            _p(sampling_loc), _p(attn_weight), B, S, M, D, Lq, L, P, int(im2col_step), dt, _p(out)),
            "ms_deform_attn_forward")
        return out

    def gemm(self, A: DeviceArray, W: DeviceArray, *, bias_n=None, bias_m=None, scale_m=None, residual=None,
             rowgroup_add=None, rows_per_group=0, act=ACT_NONE, geglu=False, alpha=1.0, out_dtype=np.float16,
             force_tile=-1, force_split=0, out=None, lda=None, ln=None) -> DeviceArray:
        """C[M,N] = epi(alpha * A[M,K] @ W[N,K]^T); 3-D inputs are batched over dim 0.  `lda` overrides the row stride of A
        (tools: overlapping rows make A cache-resident).  `ln` (test hook, odise_hip_gemm_ln): dict with any of part / parts / inv_c / eps /
        colsum / final_out / fin / rowsum / stats_out - a LayerNorm folded into the epilogue the way the CLIP towers chain their GEMMs."""
        batched = len(A.shape) == 3 or len(W.shape) == 3
        batch = (A.shape[0] if len(A.shape) == 3 else W.shape[0]) if batched else 1
        M, K = A.shape[-2:]
        N, K2 = W.shape[-2:]
        assert K == K2
        No = N // 2 if geglu else N
        oshape = (batch, M, No) if batched else (M, No)
        out = out if out is not None else self.empty(oshape, out_dtype)
        d = GemmDesc()
        d.M, d.N, d.K = M, N, K
        d.A, d.lda = A.ptr, (K if lda is None else int(lda))
        d.W, d.ldw = W.ptr, K
        d.C, d.ldc = out.ptr, No
        d.c_dtype = F32 if np.dtype(out_dtype) == np.float32 else F16
        d.bias_n = bias_n.ptr if bias_n is not None else None
        d.bias_m = bias_m.ptr if bias_m is not None else None
        d.scale_m = scale_m.ptr if scale_m is not None else None
        d.residual = residual.ptr if residual is not None else None
        d.ldr = No
        d.rowgroup_add = rowgroup_add.ptr if rowgroup_add is not None else None
        d.rows_per_group = rows_per_group
        d.act, d.geglu, d.alpha = act, int(geglu), float(alpha)
        d.batch = batch
        d.strideA = M * K if len(A.shape) == 3 else 0
        d.strideW = N * K if len(W.shape) == 3 else 0
        d.strideC = M * No
        d.strideR = M * No
        if ln is not None:
            check(self.lib.odise_hip_gemm_ln(self.h, C.byref(d), ln.get("part"), int(ln.get("parts", 0)), float(ln.get("inv_c", 0.0)),
                                             float(ln.get("eps", 0.0)), ln.get("colsum"), ln.get("final_out"), ln.get("fin"), ln.get("rowsum"),
                                             ln.get("stats_out")), "gemm_ln")
        elif force_tile >= 0 or force_split > 0:
            check(self.lib.odise_hip_gemm_forced(self.h, C.byref(d), int(force_tile), int(force_split)), "gemm_forced")
        else:
            check(self.lib.odise_hip_gemm(self.h, C.byref(d)), "gemm")
        return out

    def conv2d(self, X: DeviceArray, Wt: DeviceArray, *, stride=1, pad=None, pad_tl=None, out_hw=None, upsample2x=False,
               bias=None, residual=None, per_image_add=None, act=ACT_NONE, out_dtype=np.float16, force_tile=-1,
               force_split=0, out=None) -> DeviceArray:
        """NHWC conv: X [N,H,W,Cin] f16, Wt [Cout,KH,KW,Cin] f16 -> [N,OH,OW,Cout]."""
        N, H, W, Cin = X.shape
        Cout, KH, KW, Cin2 = Wt.shape
        assert Cin == Cin2
        if pad is None:
            pad = KH // 2
        pt, pl = pad_tl if pad_tl is not None else (pad, pad)
        Hin, Win = (2 * H, 2 * W) if upsample2x else (H, W)
        if out_hw is None:
            OH = (Hin + 2 * pad - KH) // stride + 1
            OW = (Win + 2 * pad - KW) // stride + 1
        else:
            OH, OW = out_hw
        out = out if out is not None else self.empty((N, OH, OW, Cout), out_dtype)
        d = ConvDesc()
        d.N, d.H, d.W, d.Cin = N, H, W, Cin
        d.Cout, d.KH, d.KW, d.stride = Cout, KH, KW, stride
        d.pad_t, d.pad_l, d.OH, d.OW = pt, pl, OH, OW
        d.upsample2x = int(upsample2x)
        d.X, d.Wt, d.Y = X.ptr, Wt.ptr, out.ptr
        d.y_dtype = F32 if np.dtype(out_dtype) == np.float32 else F16
        d.bias = bias.ptr if bias is not None else None
        d.residual = residual.ptr if residual is not None else None
        d.per_image_add = per_image_add.ptr if per_image_add is not None else None
        d.act = act
        if force_tile >= 0 or force_split > 0:
            check(self.lib.odise_hip_conv2d_forced(self.h, C.byref(d), int(force_tile), int(force_split)), "conv2d_forced")
        else:
            check(self.lib.odise_hip_conv2d(self.h, C.byref(d)), "conv2d")
        return out

    def conv2d_gn(self, X: DeviceArray, Wt: DeviceArray, gamma: DeviceArray, beta: DeviceArray, *, bias=None, groups=32, eps=1e-5, act=ACT_NONE,
                  force_tile=-1, force_split=0):
        """3x3 / 1x1 stride-1 conv whose epilogue reduces the GroupNorm statistics, then that GroupNorm (developer hook
        odise_hip_conv2d_gn_forced): returns (conv output, normalised output, row blocks per image; 0 = fusion declined)."""
        N, H, W, Cin = X.shape
        Cout, KH, KW, _ = Wt.shape
        y = self.empty((N, H, W, Cout), np.float16)
        yn = self.empty((N, H, W, Cout), np.float16)
        scratch = self.empty((N * ((H * W + 63) // 64) * Cout * 2,), np.float32)
        d = ConvDesc()
        d.N, d.H, d.W, d.Cin = N, H, W, Cin
        d.Cout, d.KH, d.KW, d.stride = Cout, KH, KW, 1
        d.pad_t, d.pad_l, d.OH, d.OW = KH // 2, KW // 2, H, W
        d.X, d.Wt, d.Y = X.ptr, Wt.ptr, y.ptr
        d.y_dtype = F16
        d.bias = bias.ptr if bias is not None else None
        d.act = ACT_NONE
        blocks = C.c_int(0)
        check(self.lib.odise_hip_conv2d_gn_forced(self.h, C.byref(d), int(force_tile), int(force_split), _p(gamma), _p(beta), int(groups),
                                                  C.c_float(eps), int(act), C.c_void_p(yn.ptr), C.c_void_p(scratch.ptr), C.byref(blocks)),
              "conv2d_gn_forced")
        self.sync()
        scratch.free()
        return y, yn, blocks.value

    def group_norm(self, x: DeviceArray, gamma: Optional[DeviceArray], beta: Optional[DeviceArray], groups=32, eps=1e-5,
                   act=ACT_NONE) -> DeviceArray:
        """x [N, ..., C] f16 channels-last."""
        N, Cc = x.shape[0], x.shape[-1]
        HW = int(np.prod(x.shape[1:-1]))
        y = self.empty(x.shape, np.float16)
        check(self.lib.odise_hip_group_norm(self.h, _p(x), _p(y), _p(gamma), _p(beta), N, HW, Cc, groups, C.c_float(eps), act),
              "group_norm")
        return y

    def layer_norm(self, x: DeviceArray, gamma, beta, eps=1e-5) -> DeviceArray:
        Cc = x.shape[-1]
        rows = int(np.prod(x.shape[:-1]))
        y = self.empty(x.shape, np.float16)
        check(self.lib.odise_hip_layer_norm(self.h, _p(x), _p(y), _p(gamma), _p(beta), rows, Cc, C.c_float(eps)), "layer_norm")
        return y

    def attention(self, Q: DeviceArray, K: DeviceArray, Vt: DeviceArray, heads: int, scale: float,
                  mask: Optional[DeviceArray] = None, Lk: Optional[int] = None, out: Optional[DeviceArray] = None, *,
                  B: Optional[int] = None, Lq: Optional[int] = None, D: Optional[int] = None,
                  ldq: Optional[int] = None, ldk: Optional[int] = None, ldvt: Optional[int] = None, ldo: Optional[int] = None,
                  ldmask: Optional[int] = None, strideQ: Optional[int] = None, strideK: Optional[int] = None, strideVt: Optional[int] = None,
                  strideO: Optional[int] = None, strideMask: Optional[int] = None, offQ: int = 0, offK: int = 0, offVt: int = 0, offO: int = 0,
                  offMask: int = 0) -> DeviceArray:
        """Q [B,Lq,H*D], K [B,Lk,H*D], Vt [B,H*D,ldvt] (transposed V) -> O [B,Lq,H*D] (all f16).

        The keyword arguments lay the operands out as the model's call sites do (odise_attn_desc, include/odise_hip.h): leading dimensions and
        batch strides in elements, `off*` = element offsets of the first operand element into its buffer (K = Q + C inside one q|k buffer),
        and B / Lq / D where the buffers' shapes no longer say them (`heads` stays H).  With any of them the arrays are plain buffers of any
        shape, and `out` is required unless O is packed.  Defaults: the packed layout the shapes describe."""
        explicit = not all(v is None for v in (B, Lq, D, ldq, ldk, ldvt, ldo, ldmask, strideQ, strideK, strideVt, strideO, strideMask)) \
            or bool(offQ or offK or offVt or offO or offMask)
        if not explicit:
            B, Lq, HD = Q.shape
            D = HD // heads
        else:
            assert D is not None and Lq is not None and B is not None and Lk is not None, "attention: explicit layouts name B, Lq, Lk and D"
            HD = heads * D
        Lk = Lk if Lk is not None else K.shape[1]
        if out is None:
            assert ldo in (None, HD) and strideO in (None, Lq * HD) and offO == 0, "attention: a strided O needs `out`"
        O = out if out is not None else self.empty((B, Lq, HD), np.float16)
        d = AttnDesc()
        d.B, d.H, d.Lq, d.Lk, d.D = B, heads, Lq, Lk, D
        d.ldq = HD if ldq is None else int(ldq)
        d.ldk = HD if ldk is None else int(ldk)
        d.ldvt = Vt.shape[2] if ldvt is None else int(ldvt)
        d.ldo = HD if ldo is None else int(ldo)
        d.strideQ = Lq * d.ldq if strideQ is None else int(strideQ)
        d.strideK = (Lk if explicit else K.shape[1]) * d.ldk if strideK is None else int(strideK)
        d.strideVt = (HD if explicit else Vt.shape[1]) * d.ldvt if strideVt is None else int(strideVt)
        d.strideO = Lq * d.ldo if strideO is None else int(strideO)
        d.Q, d.K, d.Vt, d.O = Q.ptr + 2 * int(offQ), K.ptr + 2 * int(offK), Vt.ptr + 2 * int(offVt), O.ptr + 2 * int(offO)
        if mask is not None:
            assert mask.dtype == np.uint8
            if not explicit:
                assert mask.shape[0] == B and mask.shape[1] == Lq
            d.ldmask = mask.shape[-1] if ldmask is None else int(ldmask)
            d.strideMask = Lq * d.ldmask if strideMask is None else int(strideMask)
            d.mask = mask.ptr + int(offMask)
        d.scale = float(scale)
        check(self.lib.odise_hip_attention(self.h, C.byref(d)), "attention")
        return O

    def nchw_to_nhwc_f16(self, x: DeviceArray, cpad: Optional[int] = None) -> DeviceArray:
        N, Cc, H, W = x.shape
        cpad = cpad or ((Cc + 7) // 8) * 8
        y = self.empty((N, H, W, cpad), np.float16)
        check(self.lib.odise_hip_nchw_f32_to_nhwc_f16(self.h, _p(x), _p(y), N, Cc, H, W, cpad), "nchw_to_nhwc")
        return y

    def nhwc_to_nchw_f32(self, x: DeviceArray) -> DeviceArray:
        N, H, W, Cc = x.shape
        y = self.empty((N, Cc, H, W), np.float32)
        check(self.lib.odise_hip_nhwc_f16_to_nchw_f32(self.h, _p(x), _p(y), N, Cc, H, W), "nhwc_to_nchw")
        return y

    def concat_channels(self, a: DeviceArray, b: DeviceArray) -> DeviceArray:
        assert a.shape[:-1] == b.shape[:-1]
        pixels = int(np.prod(a.shape[:-1]))
        y = self.empty(a.shape[:-1] + (a.shape[-1] + b.shape[-1],), np.float16)
        check(self.lib.odise_hip_concat_channels(self.h, _p(a), _p(b), _p(y), C.c_size_t(pixels), a.shape[-1], b.shape[-1]),
              "concat_channels")
        return y

    def mask_pooling(self, x: DeviceArray, mask: DeviceArray) -> DeviceArray:
        """MaskPooling.forward (odise.py:937-963): x [B,C,H,W] f32, mask [B,Q,H,W] f32 -> [B,Q,C] f32."""
        B, Cc, H, W = x.shape
        Q = mask.shape[1]
        out = self.empty((B, Q, Cc), np.float32)
        check(self.lib.odise_hip_mask_pooling(self.h, _p(x), _p(mask), _p(out), B, Cc, Q, H * W), "mask_pooling")
        return out

    # ---- eval-loop helpers (include/odise_hip.h, last section) ---------------------------------------------------------------------
    def resize_bilinear_u8(self, img: DeviceArray, out_h: int, out_w: int) -> DeviceArray:
        """uint8 [H,W,C] -> uint8 [out_h,out_w,C], bit-identical to PIL.Image.resize((out_w, out_h), BILINEAR)."""
        H, W, Cc = img.shape
        assert img.dtype == np.uint8
        out = self.empty((out_h, out_w, Cc), np.uint8)
        check(self.lib.odise_hip_resize_bilinear_u8(self.h, _p(img), H, W, Cc, _p(out), int(out_h), int(out_w)), "resize_bilinear_u8")
        return out

    def u8_hwc_to_f32_chw(self, img: DeviceArray, scale: float = 1.0) -> DeviceArray:
        H, W, Cc = img.shape
        out = self.empty((Cc, H, W), np.float32)
        check(self.lib.odise_hip_u8_hwc_to_f32_chw(self.h, _p(img), _p(out), H, W, Cc, C.c_float(scale)), "u8_hwc_to_f32_chw")
        return out

    def u8_hwc_to_f32_chw_padded(self, img: DeviceArray, Hp: int, Wp: int, scale: float = 1.0, out: Optional[DeviceArray] = None) -> DeviceArray:
        """uint8 [H,W,C] -> fp32 [C,Hp,Wp] with the image in the top-left corner and zeros elsewhere (ImageList.from_tensors)."""
        H, W, Cc = img.shape
        if out is None:
            out = self.empty((Cc, Hp, Wp), np.float32)
        assert out.nbytes == Cc * Hp * Wp * 4
        check(self.lib.odise_hip_u8_hwc_to_f32_chw_padded(self.h, _p(img), _p(out), H, W, Cc, int(Hp), int(Wp), C.c_float(scale)), "u8_hwc_to_f32_chw_padded")
        return out

    def semantic_confusion(self, sem_seg: DeviceArray, gt: DeviceArray, conf: Optional[DeviceArray] = None) -> DeviceArray:
        """sem_seg f32 [K,H,W], gt int32 [H,W] (ignore label already mapped outside [0,K)) -> int64 [(K+1),(K+1)] accumulated into conf."""
        K = sem_seg.shape[0]
        npix = int(np.prod(sem_seg.shape[1:]))
        if conf is None:
            conf = self.zeros((K + 1, K + 1), np.int64)
        check(self.lib.odise_hip_semantic_confusion(self.h, _p(sem_seg), _p(gt), K, npix, _p(conf)), "semantic_confusion")
        return conf

    # Boundary IoU counters of SemSegEvaluator (include/odise_hip.h odise_hip_boundary_radius ..; host restatement: odise_amd/sem_boundary.py)
    def boundary_radius(self, H: int, W: int) -> int:
        """The evaluator's erosion count for an H x W picture: max(1, int(round(0.02 * sqrt(H*H + W*W))))."""
        r = self.lib.odise_hip_boundary_radius(int(H), int(W))
        check(min(r, 0), "boundary_radius")
        return r

    def label_boundary(self, labels: DeviceArray, K: int, radius: int = 0, out: Optional[DeviceArray] = None) -> DeviceArray:
        """labels int32 [H,W] (values outside [0,K] count as K) -> int32 [H,W] _mask_to_boundary(labels); radius <= 0: the formula."""
        H, W = labels.shape
        assert labels.dtype == np.int32
        if out is None:
            out = self.empty((H, W), np.int32)
        assert out.dtype == np.int32 and out.shape == (H, W)
        check(self.lib.odise_hip_label_boundary(self.h, _p(labels), int(K), H, W, int(radius), _p(out)), "label_boundary")
        return out

    def semantic_boundary_confusion(self, sem_seg: DeviceArray, gt: DeviceArray, conf: Optional[DeviceArray] = None,
                                    b_conf: Optional[DeviceArray] = None, radius: int = 0):
        """One SemSegEvaluator.process step: sem_seg f32 [K,H,W], gt int32 [H,W] -> (conf, b_conf), int64 [(K+1),(K+1)] each, accumulated.
        conf None: only the boundary matrix is counted (None is returned in its place); b_conf None: a fresh zeroed matrix."""
        K, H, W = sem_seg.shape
        assert gt.shape == (H, W) and gt.dtype == np.int32 and sem_seg.dtype == np.float32
        if b_conf is None:
            b_conf = self.zeros((K + 1, K + 1), np.int64)
        check(self.lib.odise_hip_semantic_boundary_confusion(self.h, _p(sem_seg), _p(gt), K, H, W, int(radius), _p(conf), _p(b_conf)),
              "semantic_boundary_confusion")
        return conf, b_conf

    # ---- the whole SemSegEvaluator.process step (include/odise_hip.h odise_hip_semantic_eval; host restatement: odise_amd/semseg_eval.py) ----
    def semantic_eval_async(self, pred: DeviceArray, K: Optional[int] = None, gt: Optional[DeviceArray] = None, conf: Optional[DeviceArray] = None,
                            b_conf: Optional[DeviceArray] = None, flags: Optional[DeviceArray] = None, radius: int = 0, rle: bool = True,
                            max_classes: Optional[int] = None, capacity: Optional[int] = None, bufs=None,
                            pq_stats: Optional[DeviceArray] = None) -> "SemSegPending":
        """Enqueue one SemSegEvaluator.process step: pred = labels int32 [H,W] (needs K) or sem_seg float32 [K,H,W]; gt int32 [H,W] with the
        ignore label already mapped to K.  conf / b_conf int64 [(K+1),(K+1)] are added to (with a gt and neither given, a fresh zeroed conf
        is counted; b_conf only when given), flags int32 [1] is OR-ed into (a fresh zeroed one when none is given).  rle: also the per-class
        COCO RLE strings, at most max_classes (default MAX_SEGMENTS) of them at first; `SemSegPending.result()` enqueues the call again when
        the strings did not fit the capacity or more classes are present - it reads `pred` again, so `pred` must hold the picture until
        `settle()` or `result()` has run (call `settle()` before a pooled buffer is handed on).  bufs =(bytes uint8 [capacity], meta int32 [1 + max_classes],
        offsets-and-area int64 [2 max_classes + 1]) device arrays to use instead of fresh ones (a retry still allocates its own).
        pq_stats [K] records (panoptic_quality.STAT_DTYPE; needs a gt): the first launch is `odise_hip_semantic_eval_pq` and also adds the
        picture's semantic PQ statistics (`semantic_pq`) from the same label map; a retry never counts."""
        _labels, _sem, K, H, W = _labels_or_scores(pred, K)
        assert gt is None or (gt.dtype == np.int32 and tuple(gt.shape) == (H, W)), "gt must be int32 [H,W]"
        if gt is not None and conf is None and b_conf is None and pq_stats is None:
            conf = self.zeros((K + 1, K + 1), np.int64)
        for m in (conf, b_conf):
            assert m is None or (m.dtype == np.int64 and int(np.prod(m.shape)) == (K + 1) * (K + 1)), "conf / b_conf must be int64 [(K+1),(K+1)]"
        flags = self._flags_buffer(flags)
        if pq_stats is not None:
            from .panoptic_quality import STAT_DTYPE
            assert gt is not None and pq_stats.dtype == STAT_DTYPE and pq_stats.shape == (K,), "pq_stats needs a gt and [K] records"
        return SemSegPending(self, pred, K, (H, W), gt, conf, b_conf, flags, int(radius), bool(rle), max_classes, capacity, bufs, pq_stats)

    @staticmethod
    def sem_rle_bytes(hw) -> int:
        """Default string capacity of a picture's semantic RLE, all classes together.  The classes partition the picture, so the strings
        hold two runs (one to three characters each for a smooth map) per change of label along the columns, whatever the number of
        classes: a byte per four pixels covers a change every ~16 pixels of every column; a busier map costs the retry."""
        return max(4096, int(hw[0]) * int(hw[1]) // 4)

    def semantic_eval(self, pred: DeviceArray, K: Optional[int] = None, gt: Optional[DeviceArray] = None, **kw):
        """`semantic_eval_async(...).result()`: (classes int32 [n], RLE dicts [n], area int64 [n]) of the classes present, ascending."""
        return self.semantic_eval_async(pred, K, gt, **kw).result()

    # PQ of a semantic segmentation (include/odise_hip.h odise_hip_semantic_pq; host restatement: odise_amd/semseg_pq.py)
    def semantic_pq(self, pred: DeviceArray, gt: DeviceArray, K: Optional[int] = None, stats: Optional[DeviceArray] = None,
                    flags: Optional[DeviceArray] = None):
        """One picture of the PQ-for-semantic-segmentation metric, enqueued: pred = labels int32 [H,W] (needs K) or sem_seg float32
        [K,H,W] (first-maximum arg-max); gt int32 [H,W] with the ignore label already mapped to K (anything outside [0,K] counts as K)
        -> (stats, flags): `stats` [K] records (panoptic_quality.STAT_DTYPE) added to, `flags` int32 [1] OR-ed into (1 = a label
        outside [0,K): that picture adds nothing); fresh zeroed ones when none are given."""
        labels, sem, K, H, W = _labels_or_scores(pred, K)
        assert gt.dtype == np.int32 and tuple(gt.shape) == (H, W), "gt must be int32 [H,W]"
        stats, flags = self._stats_buffer(K, stats), self._flags_buffer(flags)
        check(self.lib.odise_hip_semantic_pq(self.h, _p(labels), _p(sem), _p(gt), K, H, W, _p(stats), _p(flags)), "semantic_pq")
        return stats, flags

    def pair_histogram(self, a: DeviceArray, b: DeviceArray, na: int, nb: int, hist: Optional[DeviceArray] = None) -> DeviceArray:
        npix = int(np.prod(a.shape))
        if hist is None:
            hist = self.zeros((na, nb), np.int32)
        check(self.lib.odise_hip_pair_histogram(self.h, _p(a), _p(b), npix, int(na), int(nb), _p(hist)), "pair_histogram")
        return hist

    # ---- panoptic quality statistics (include/odise_hip.h odise_hip_panoptic_quality; host restatement: odise_amd/panoptic_quality.py) ----
    def panoptic_quality(self, pred_ids: DeviceArray, pred_segments: DeviceArray, gt: DeviceArray, gt_segments, num_categories: int,
                         stats: Optional[DeviceArray] = None, flags: Optional[DeviceArray] = None):
        """One picture of COCOPanopticEvaluator.process + pq_compute_single_core, enqueued: pred_ids int32 [H,W] panoptic ids and
        pred_segments int32 [n | n x (id, isthing, category)] (the two parts of a panoptic record), gt uint8 [H,W,3] (the annotation PNG
        as decoded) or int32 [H,W] ids, gt_segments HOST rows (id, category, iscrowd, area) -> (stats, flags): `stats` [num_categories]
        records (panoptic_quality.STAT_DTYPE) added to, `flags` int32 [1] OR-ed into; fresh zeroed ones when none are given."""
        d, _table, stats, flags = self._pq_desc(pred_ids, pred_segments, gt, gt_segments, num_categories, stats, flags)
        check(self.lib.odise_hip_panoptic_quality(self.h, C.byref(d)), "panoptic_quality")
        return stats, flags

    def _stats_buffer(self, n: int, stats: Optional[DeviceArray]) -> DeviceArray:
        """`stats` [n] records of panoptic_quality.STAT_DTYPE; a fresh zeroed one when None."""
        from .panoptic_quality import STAT_DTYPE
        if stats is None:
            stats = self.zeros((int(n),), STAT_DTYPE)
        assert stats.dtype == STAT_DTYPE and stats.shape == (int(n),)
        return stats

    def _flags_buffer(self, flags: Optional[DeviceArray]) -> DeviceArray:
        """`flags` int32 [1]; a fresh zeroed one when None."""
        if flags is None:
            flags = self.zeros((1,), np.int32)
        assert flags.dtype == np.int32
        return flags

    def _pq_desc(self, pred_ids, pred_segments, gt, gt_segments, num_categories, stats, flags):
        """-> (PqDesc, the host table it points to, stats, flags) of the arguments of `panoptic_quality`."""
        from ._lib import PqDesc
        if gt.dtype == np.uint8:
            assert len(gt.shape) == 3 and gt.shape[2] == 3, gt.shape
            layout = 0
        else:
            assert gt.dtype == np.int32 and len(gt.shape) == 2, (gt.dtype, gt.shape)
            layout = 1
        H, W = gt.shape[:2]
        assert pred_ids.dtype == np.int32 and int(np.prod(pred_ids.shape)) == H * W, (pred_ids.dtype, pred_ids.shape, (H, W))
        assert pred_segments.dtype == np.int32
        table = np.ascontiguousarray(np.asarray(gt_segments, np.int64).reshape(-1, 4), np.int32)
        stats, flags = self._stats_buffer(num_categories, stats), self._flags_buffer(flags)
        d = PqDesc()
        d.H, d.W, d.pred_ids, d.pred_segments, d.gt, d.gt_layout = H, W, pred_ids.ptr, pred_segments.ptr, gt.ptr, layout
        d.gt_segments, d.n_gt, d.num_categories = table.ctypes.data, table.shape[0], int(num_categories)
        d.stats, d.flags = stats.ptr, flags.ptr
        return d, table, stats, flags

    def panoptic_quality_record(self, record: DeviceArray, hw, gt: DeviceArray, gt_segments, num_categories: int,
                                stats: Optional[DeviceArray] = None, flags: Optional[DeviceArray] = None):
        """`panoptic_quality` of a panoptic record int32 [h*w | 1 | 3*MAX_SEGMENTS] as odise_hip_infer / postprocess_batch leave it on the
        device (also a row of the exchange buffer): the map and the table are two offsets into it, nothing travels to the host."""
        from ._lib import split_record
        ids, table = split_record(record, hw)
        return self.panoptic_quality(ids, table, gt, gt_segments, num_categories, stats, flags)

    # Boundary PQ beside PQ (include/odise_hip.h odise_hip_panoptic_quality_boundary; host restatement: panoptic_quality.image_boundary_stats)
    def panoptic_quality_boundary(self, pred_ids: DeviceArray, pred_segments: DeviceArray, gt: DeviceArray, gt_segments, num_categories: int,
                                  stats: Optional[DeviceArray] = None, b_stats: Optional[DeviceArray] = None,
                                  flags: Optional[DeviceArray] = None, radius: int = 0):
        """`panoptic_quality` with the Boundary PQ statistics beside it, one call: -> (stats, b_stats, flags).  `stats` receives exactly
        what `panoptic_quality` adds, `b_stats` [num_categories] records the matching on min(mask IoU, boundary IoU); radius <= 0: the
        formula of `boundary_radius`.  Fresh zeroed accumulators when none are given."""
        from ._lib import PqBoundaryTask
        d, _table, stats, flags = self._pq_desc(pred_ids, pred_segments, gt, gt_segments, num_categories, stats, flags)
        b_stats = self._stats_buffer(num_categories, b_stats)
        b = PqBoundaryTask()
        b.stats, b.radius = b_stats.ptr, int(radius)
        check(self.lib.odise_hip_panoptic_quality_boundary(self.h, C.byref(d), C.byref(b)), "panoptic_quality_boundary")
        return stats, b_stats, flags

    def panoptic_quality_boundary_record(self, record: DeviceArray, hw, gt: DeviceArray, gt_segments, num_categories: int,
                                         stats: Optional[DeviceArray] = None, b_stats: Optional[DeviceArray] = None,
                                         flags: Optional[DeviceArray] = None, radius: int = 0):
        """`panoptic_quality_boundary` of a panoptic record, as `panoptic_quality_record`."""
        from ._lib import split_record
        ids, table = split_record(record, hw)
        return self.panoptic_quality_boundary(ids, table, gt, gt_segments, num_categories, stats, b_stats, flags, radius)

    def segment_boundaries(self, ids: DeviceArray, table, radius: int = 0, out: Optional[DeviceArray] = None, with_area: bool = False):
        """ids int32 [H,W] (device), table: the ids of at most 254 segments (host or device int32) -> uint8 [H,W], 1 where a pixel lies on
        the boundary of its own segment (odise_hip_segment_boundaries; byte for byte panoptic_quality.segment_boundaries); pixels of id 0
        and of ids absent from the table are 0.  with_area adds the boundary pixels of each table row, int64 [n] (None for an empty
        table)."""
        H, W = ids.shape
        assert ids.dtype == np.int32
        if not isinstance(table, DeviceArray):
            table = np.ascontiguousarray(np.asarray(table, np.int64).reshape(-1), np.int32)
            table = self.to_device(table) if table.size else None
        n = int(np.prod(table.shape)) if table is not None else 0
        assert table is None or table.dtype == np.int32
        if out is None:
            out = self.empty((H, W), np.uint8)
        assert out.dtype == np.uint8 and out.shape == (H, W)
        area = self.empty((n,), np.int64) if with_area and n else None
        check(self.lib.odise_hip_segment_boundaries(self.h, _p(ids), H, W, _p(table), n, int(radius), _p(out), _p(area)), "segment_boundaries")
        return (out, area) if with_area else out

    # ---- drawing a panoptic result (include/odise_hip.h odise_hip_connected_components ..; host restatement: odise_amd/visualize.py) ----
    def connected_components(self, labels: DeviceArray, out: Optional[DeviceArray] = None) -> DeviceArray:
        """labels int32 [H,W] -> int32 [H,W]: the smallest row-major index of the pixel's 8-connected component of equal labels,
        -1 where labels <= 0."""
        H, W = labels.shape
        assert labels.dtype == np.int32
        if out is None:
            out = self.empty((H, W), np.int32)
        assert out.dtype == np.int32 and out.shape == (H, W)
        check(self.lib.odise_hip_connected_components(self.h, _p(labels), H, W, _p(out)), "connected_components")
        return out

    def segment_anchors(self, pred_ids: DeviceArray, pred_segments: DeviceArray, small_area: int = 1000, large_area: int = 120000,
                        cap: int = 256, anchors: Optional[DeviceArray] = None, n_anchors: Optional[DeviceArray] = None):
        """Label anchors of a panoptic result, enqueued: pred_ids int32 [H,W], pred_segments int32 [n | n x (id, isthing, category)]
        -> (anchors [cap] records of visualize.ANCHOR_DTYPE, n_anchors int32 [1] = all that were found)."""
        from ._lib import AnchorDesc
        from .visualize import ANCHOR_DTYPE
        H, W = pred_ids.shape
        assert pred_ids.dtype == np.int32 and pred_segments.dtype == np.int32
        if anchors is None:
            anchors = self.zeros((int(cap),), ANCHOR_DTYPE)
        if n_anchors is None:
            n_anchors = self.zeros((1,), np.int32)
        assert anchors.dtype == ANCHOR_DTYPE and anchors.shape[0] >= max(int(cap), 0) and n_anchors.dtype == np.int32
        d = AnchorDesc()
        d.H, d.W, d.pred_ids, d.pred_segments = H, W, pred_ids.ptr, pred_segments.ptr
        d.small_area, d.large_area, d.anchors, d.cap, d.n_anchors = int(small_area), int(large_area), anchors.ptr, int(cap), n_anchors.ptr
        check(self.lib.odise_hip_segment_anchors(self.h, C.byref(d)), "segment_anchors")
        return anchors, n_anchors

    def panoptic_overlay(self, image: DeviceArray, pred_ids: DeviceArray, pred_segments: DeviceArray, colors: DeviceArray,
                         alpha256: int = 128, edge_rgb=(0, 0, 0), out: Optional[DeviceArray] = None) -> DeviceArray:
        """image uint8 [H,W,3] -> out uint8 [H,W,3] (may be `image`): segments blended with colors uint8 [n,3], outlines in edge_rgb."""
        from ._lib import OverlayDesc
        H, W = pred_ids.shape
        assert image.dtype == np.uint8 and image.shape == (H, W, 3), (image.dtype, image.shape)
        assert pred_ids.dtype == np.int32 and pred_segments.dtype == np.int32 and colors.dtype == np.uint8
        if out is None:
            out = self.empty((H, W, 3), np.uint8)
        assert out.dtype == np.uint8 and out.shape == (H, W, 3)
        d = OverlayDesc()
        d.H, d.W, d.image, d.pred_ids, d.pred_segments, d.colors = H, W, image.ptr, pred_ids.ptr, pred_segments.ptr, colors.ptr
        d.alpha256, d.out = int(alpha256), out.ptr
        d.edge_rgb[0], d.edge_rgb[1], d.edge_rgb[2] = (int(c) & 255 for c in edge_rgb)
        check(self.lib.odise_hip_panoptic_overlay(self.h, C.byref(d)), "panoptic_overlay")
        return out

    # ---- test-time augmentation of the semantic head (include/odise_hip.h odise_hip_tta_*; driver: odise_amd/tta.py) -----------------------
    def tta_create(self, out_hw, K: int, Q: int, max_views: int) -> "SemanticTTA":
        """A handle that sums up to `max_views` views of a picture whose result has out_hw = (H, W), K classes, Q queries."""
        return SemanticTTA(self, out_hw, K, Q, max_views)

    def hflip_u8_hwc(self, img: DeviceArray, out: Optional[DeviceArray] = None) -> DeviceArray:
        """uint8 [H,W,C] mirrored left to right (HFlipTransform on the resized picture)."""
        H, W, Cc = img.shape
        assert img.dtype == np.uint8
        if out is None:
            out = self.empty((H, W, Cc), np.uint8)
        assert out.nbytes == H * W * Cc
        check(self.lib.odise_hip_hflip_u8_hwc(self.h, _p(img), _p(out), H, W, Cc), "hflip_u8_hwc")
        return out

    # ---- colours of things across frames (include/odise_hip.h odise_hip_track_*; host restatement: odise_amd/video.py) -------------------
    def track_create(self, hw, ttl: int = 8, pool=None) -> "Tracker":
        """A tracker for frames of hw = (H, W): pool uint8 [P,3] on the host (video.default_pool() when None)."""
        return Tracker(self, hw, ttl, pool)

    def track_frame(self, tracker: "Tracker", pred_ids: DeviceArray, pred_segments: DeviceArray, colors: DeviceArray,
                    live: Optional[DeviceArray] = None, n_live: Optional[DeviceArray] = None, iou: Optional[DeviceArray] = None,
                    live_cap: Optional[int] = None, iou_cap: Optional[int] = None) -> DeviceArray:
        """One frame, enqueued: pred_ids int32 [H,W] and pred_segments int32 [n | n x (id, isthing, category)] (the two parts of a panoptic
        record), colors uint8 [MAX_SEGMENTS,3] in/out (the rows of the frame's instances are rewritten).  Optional dumps: live [cap]
        records of video.TRACK_ROW_DTYPE with n_live int32 [1], iou float64 [cap, MAX_SEGMENTS]."""
        from ._lib import MAX_SEGMENTS, TrackDesc
        H, W = pred_ids.shape
        assert pred_ids.dtype == np.int32 and pred_segments.dtype == np.int32
        assert colors.dtype == np.uint8 and colors.nbytes >= 3 * MAX_SEGMENTS, (colors.dtype, colors.shape)
        d = TrackDesc()
        d.track, d.H, d.W, d.pred_ids, d.pred_segments, d.colors = tracker.handle, H, W, pred_ids.ptr, pred_segments.ptr, colors.ptr
        _fill_track_dumps(d, live, n_live, iou, live_cap, iou_cap)
        check(self.lib.odise_hip_track_frame(self.h, C.byref(d)), "track_frame")
        return colors

    def _fill_track_colors(self, d, topk: int, colors: Optional[DeviceArray], edge_colors: Optional[DeviceArray]) -> DeviceArray:
        """colors uint8 [topk,3] by table index (zeros when None) and the optional edge_colors of InstTrackDesc / BoxTrackDesc -> colors."""
        if colors is None:
            colors = self.zeros((topk, 3), np.uint8)
        assert colors.dtype == np.uint8 and colors.nbytes >= 3 * topk, (colors.dtype, colors.shape)
        d.colors = colors.ptr
        if edge_colors is not None:
            assert edge_colors.dtype == np.uint8 and edge_colors.nbytes >= 3 * topk, (edge_colors.dtype, edge_colors.shape)
            d.edge_colors = edge_colors.ptr
        return colors

    # ---- colours of overlapping instance masks across frames (odise_hip_inst_track_*; host restatement: video.InstanceColorTracker) -----
    def inst_track_create(self, hw, topk: int, ttl: int = 8, pool=None) -> "InstTracker":
        """A tracker for selections of `topk` instance masks of hw = (H, W): pool uint8 [P,3] on the host (video.default_pool() when None).
        It owns (ttl + 1) * topk * W * ceil(H / 64) * 8 bytes of packed masks."""
        return InstTracker(self, hw, topk, ttl, pool)

    def inst_track_frame(self, tracker: "InstTracker", table_row=None, scores_row=None, masks: Optional[DeviceArray] = None, b: int = 0,
                         pad_hw=(0, 0), img_hw=(0, 0), min_score: float = 0.0, colors: Optional[DeviceArray] = None,
                         edge_colors: Optional[DeviceArray] = None, live: Optional[DeviceArray] = None, n_live: Optional[DeviceArray] = None,
                         iou: Optional[DeviceArray] = None, live_cap: Optional[int] = None, iou_cap: Optional[int] = None) -> DeviceArray:
        """One frame, enqueued.  Detections as in `instance_draw`: the selection table_row [1 + 2 topk] / scores_row [topk] of image b of
        the last head forward, or dense `masks` [topk, h, w] (table_row / scores_row then optional).  colors uint8 [topk,3] in/out by table
        index (allocated as zeros when None; the rows of the frame's instances are rewritten), edge_colors the same for the outline
        colours.  Optional dumps as in `track_frame`: live [cap] records of video.TRACK_ROW_DTYPE with n_live int32 [1], iou float64
        [cap, MAX_SEGMENTS]."""
        from ._lib import InstTrackDesc
        d = InstTrackDesc()
        d.track, d.min_score = tracker.handle, float(min_score)
        _fill_inst_source(d, "inst_track_frame", tracker.hw, tracker.topk, table_row, scores_row, masks, b, pad_hw, img_hw)
        colors = self._fill_track_colors(d, tracker.topk, colors, edge_colors)
        _fill_track_dumps(d, live, n_live, iou, live_cap, iou_cap)
        check(self.lib.odise_hip_inst_track_frame(self.h, C.byref(d)), "inst_track_frame")
        return colors

    # ---- colours of instances that carry boxes across frames (odise_hip_box_track_*; host restatement: video.BoxColorTracker) -----------
    def box_track_create(self, topk: int, ttl: int = 8, pool=None) -> "BoxTracker":
        """A tracker for selections of `topk` instance boxes: pool uint8 [P,3] on the host (video.default_pool() when None).  It owns no
        pixels: 800 live rows and their boxes."""
        return BoxTracker(self, topk, ttl, pool)

    def box_track_frame(self, tracker: "BoxTracker", boxes: DeviceArray, table_row=None, scores_row=None, min_score: float = 0.0,
                        colors: Optional[DeviceArray] = None, edge_colors: Optional[DeviceArray] = None, live: Optional[DeviceArray] = None,
                        n_live: Optional[DeviceArray] = None, iou: Optional[DeviceArray] = None, live_cap: Optional[int] = None,
                        iou_cap: Optional[int] = None) -> DeviceArray:
        """One frame, enqueued (one launch): boxes float32 [topk,4] XYXY on the device (as `instance_boxes` returns them), the selection
        table_row [1 + 2 topk] / scores_row [topk] (both optional: every box counts, every class is 0, no score test).  colors /
        edge_colors and the dumps as in `inst_track_frame`."""
        from ._lib import BoxTrackDesc
        topk = tracker.topk
        assert boxes.dtype == np.float32 and boxes.nbytes >= 16 * topk, (boxes.dtype, boxes.shape)
        d = BoxTrackDesc()
        d.track, d.boxes, d.inst_table, d.inst_scores, d.topk, d.min_score = tracker.handle, boxes.ptr, _ptr(table_row), _ptr(scores_row), topk, float(min_score)
        colors = self._fill_track_colors(d, topk, colors, edge_colors)
        _fill_track_dumps(d, live, n_live, iou, live_cap, iou_cap)
        check(self.lib.odise_hip_box_track_frame(self.h, C.byref(d)), "box_track_frame")
        return colors

    # ---- drawing instance and semantic results (include/odise_hip.h odise_hip_instance_draw / odise_hip_semantic_record) ----------------
    def instance_draw_boxes(self, out_hw, topk: int, boxes: DeviceArray, box_width: int = 1, box_alpha256: int = 128, small_area: int = 1000,
                            **kw) -> dict:
        """`instance_draw` for instances that carry boxes (odise_hip_instance_draw_boxes: overlay_instances(boxes=, masks=)): boxes
        float32 [topk,4] XYXY on the device; a frame of box_width pixels per box, the draw order by box area, the anchors on the box
        corners.  Every other argument and the result are `instance_draw`'s."""
        from ._lib import InstBoxDraw
        assert boxes.dtype == np.float32 and boxes.nbytes >= 16 * int(topk), (boxes.dtype, boxes.shape)
        bx = InstBoxDraw()
        bx.boxes, bx.box_width, bx.box_alpha256, bx.small_area = boxes.ptr, int(box_width), int(box_alpha256), int(small_area)
        return self.instance_draw(out_hw, topk, _boxes=bx, **kw)

    def instance_draw(self, out_hw, topk: int, table_row=None, scores_row=None, masks: Optional[DeviceArray] = None, b: int = 0, pad_hw=(0, 0),
                      img_hw=(0, 0), min_score: float = 0.0, image: Optional[DeviceArray] = None, colors: Optional[DeviceArray] = None,
                      edge_colors: Optional[DeviceArray] = None, alpha256: int = 128, want=("out", "anchors", "order"), out=None, anchors=None,
                      order=None, _boxes=None) -> dict:
        """Enqueue odise_hip_instance_draw.  Detections as in `instance_eval`: the selection table_row [1 + 2 topk] / scores_row [topk]
        of image b of the last head forward, or dense `masks` [topk, h, w] (table_row / scores_row then optional).  `want` names the
        outputs; buffers given for them are used, others are allocated -> {"out": uint8 [h,w,3], "anchors": visualize.ANCHOR_DTYPE
        [topk], "order": int32 [topk]} (the ones asked for)."""
        from ._lib import InstDrawDesc
        from .visualize import ANCHOR_DTYPE
        h, w, topk = int(out_hw[0]), int(out_hw[1]), int(topk)
        d = InstDrawDesc()
        d.min_score, d.alpha256 = float(min_score), int(alpha256)
        _fill_inst_source(d, "instance_draw", (h, w), topk, table_row, scores_row, masks, b, pad_hw, img_hw)
        res = {}
        if "out" in want:
            assert image is not None and image.dtype == np.uint8 and tuple(image.shape) == (h, w, 3), "instance_draw: image uint8 [h,w,3]"
            res["out"] = out if out is not None else self.empty((h, w, 3), np.uint8)
            d.image, d.colors, d.edge_colors, d.out = image.ptr, _ptr(colors), _ptr(edge_colors), res["out"].ptr
        if "anchors" in want:
            res["anchors"] = anchors if anchors is not None else self.empty((topk,), ANCHOR_DTYPE)
            d.anchors = res["anchors"].ptr
        if "order" in want:
            res["order"] = order if order is not None else self.empty((topk,), np.int32)
            d.order = res["order"].ptr
        if _boxes is not None:
            check(self.lib.odise_hip_instance_draw_boxes(self.h, C.byref(d), C.byref(_boxes)), "instance_draw_boxes")
        else:
            check(self.lib.odise_hip_instance_draw(self.h, C.byref(d)), "instance_draw")
        return res

    def semantic_record(self, labels_or_sem_seg: DeviceArray, K: Optional[int] = None, out: Optional[DeviceArray] = None) -> DeviceArray:
        """labels int32 [H,W] (needs K) or sem_seg float32 [K,H,W] -> the panoptic record int32 [H*W + 1 + 3*MAX_SEGMENTS] of the semantic
        result (ids = category + 1, rows (id, 0, category) by descending pixel count), enqueued."""
        from ._lib import record_len
        labels, sem, K, H, W = _labels_or_scores(labels_or_sem_seg, K)
        if out is None:
            out = self.empty((record_len(H, W),), np.int32)
        assert out.dtype == np.int32 and int(np.prod(out.shape)) >= record_len(H, W)
        check(self.lib.odise_hip_semantic_record(self.h, _p(labels), _p(sem), K, H, W, _p(out)), "semantic_record")
        return out

    # ---- COCO RLE of instance masks (segm evaluation; include/odise_hip.h odise_hip_rle_encode / odise_hip_instance_rle) ----------------
    # Default string capacity per mask.  A string has one to seven characters per run and most runs of a real mask take two or three, so
    # 8 KiB holds a mask with ~3000 runs - a blob spanning ~1500 columns; a selection that needs more costs one more pass (the retry).
    RLE_BYTES_PER_MASK = 8192

    def rle_encode_async(self, masks: DeviceArray, capacity: Optional[int] = None, bufs=None, grow=None) -> "RlePending":
        """Enqueue the COCO RLE of masks [n, h, w] (float32, or uint8 / bool; nonzero = 1) on the context's stream."""
        n, h, w = masks.shape
        dt = _mask_dtype(masks, "rle_encode")

        def launch(buf, cap, off, area):
            check(self.lib.odise_hip_rle_encode(self.h, _p(masks), dt, n, h, w, _p(buf), int(cap), _p(off), _p(area)), "rle_encode")
        return RlePending(self, n, (h, w), launch, capacity, bufs, grow=grow)

    def rle_encode(self, masks: DeviceArray, capacity: Optional[int] = None):
        """-> ([{"size": [h, w], "counts": str}] per mask, area int64 [n]), the bytes of pycocotools' mask.encode."""
        return self.rle_encode_async(masks, capacity).result()

    def instance_rle_async(self, b: int, table_row, topk: int, pad_hw, img_hw, out_hw, capacity: Optional[int] = None, bufs=None,
                           grow=None) -> "RlePending":
        """Enqueue the RLE of image b's instance selection of the last head forward straight from its mask logits; table_row = that image's
        device row [1 + 2 * topk] int32 of the instance table (DeviceArray or pointer)."""
        topk = int(topk)

        def launch(buf, cap, off, area):
            check(self.lib.odise_hip_instance_rle(self.h, int(b), table_row, topk, int(pad_hw[0]), int(pad_hw[1]), int(img_hw[0]), int(img_hw[1]),
                                                  int(out_hw[0]), int(out_hw[1]), _p(buf), int(cap), _p(off), _p(area)), "instance_rle")
        return RlePending(self, topk, tuple(int(v) for v in out_hw), launch, capacity, bufs, trim=True, grow=grow)

    def instance_rle(self, b: int, table_row, topk: int, pad_hw, img_hw, out_hw, capacity: Optional[int] = None):
        """-> (RLE dicts of the selected instances in table order, area int64 [count])."""
        return self.instance_rle_async(b, table_row, topk, pad_hw, img_hw, out_hw, capacity).result()

    def polygon_rle(self, annotations_polys, hw, capacity: Optional[int] = None):
        """pycocotools' annToRLE on the device (odise_hip_polygon_rle): annotations_polys = [[polygon, ..] per annotation], a polygon a flat
        list x0 y0 x1 y1 ..; an annotation is the union of its polygons, one without polygons the empty mask -> (RLE dicts of size hw,
        area int64 [n]): the bytes of mask.merge(mask.frPyObjects(polygons, h, w)).  Malformed polygons raise ValueError on the host.
        The polygons go up as one packed upload, which waits for the stream."""
        from . import coco_poly
        xy, poly_offsets, ann_polys = coco_poly.pack_polygons(annotations_polys)
        n, n_poly, h, w = len(ann_polys) - 1, len(poly_offsets) - 1, int(hw[0]), int(hw[1])
        buf = self.to_device(np.concatenate([poly_offsets.view(np.uint8), xy.view(np.uint8), ann_polys.view(np.uint8)]))
        d_off, d_xy = buf.view((n_poly + 1,), np.int64), buf.view((xy.size,), np.float64, poly_offsets.nbytes)
        d_ann = buf.view((n + 1,), np.int32, poly_offsets.nbytes + xy.nbytes)
        flags = self.zeros((1,), np.int32)

        def launch(out, cap, off, area):
            check(self.lib.odise_hip_polygon_rle(self.h, _p(d_xy), _p(d_off), _p(d_ann), n, n_poly, h, w, _p(out), int(cap), _p(off), _p(area),
                                                 _p(flags)), "polygon_rle")
        rles, area = RlePending(self, n, (h, w), launch, capacity).result()
        f = int(flags.numpy()[0])
        if f:
            raise RuntimeError(f"polygon_rle: malformed polygon(s) (flags {f})")
        return rles, area

    # ---- segm evaluation of instance masks (include/odise_hip.h odise_hip_mask_iou / odise_hip_instance_eval; host restatement:
    # odise_amd/instance_eval.py) ------------------------------------------------------------------------------------------------------
    def instance_gt_to_device(self, gt_table, runs, offsets, xy=None, poly_offsets=None, gt_polys=None, boxes=None, lvis_bits=None) -> dict:
        """The ground truth of one picture (instance_eval.gt_rows) as ONE packed upload: offsets int64 [n_gt + 1] | table int32 [n_gt, 3] |
        runs uint32 -> {"n_gt", "offsets", "rows", "runs"} (views of one device buffer).  With the polygon part of
        `gt_rows(..., polygons=True)` the same upload carries poly_offsets int64 | xy float64 in front of the table and gt_polys int32
        behind it, and the dict gains {"n_poly", "xy", "poly_offsets", "gt_polys"}.  With `boxes` (instance_eval.gt_boxes: float64
        [n_gt, 4] XYWH) the same upload carries them in front of the table and the dict gains {"boxes"}.  With `lvis_bits` = (neg,
        not_exhaustive), two uint32 [ceil(K / 32)] bitsets (lvis_eval.category_bits), it carries those too and the dict gains
        {"neg_bits", "not_exhaustive_bits"}.  The upload waits for the stream."""
        runs, offsets = np.ascontiguousarray(runs, np.uint32), np.ascontiguousarray(offsets, np.int64)
        if gt_table is None:                                             # masks alone (the frames of the video evaluator): "rows" is empty
            table, n_gt = np.zeros((0, 3), np.int32), offsets.size - 1
        else:
            table = np.ascontiguousarray(np.asarray(gt_table, np.int32).reshape(-1, 3))
            n_gt = table.shape[0]
        assert offsets.shape == (n_gt + 1,) and int(offsets[-1]) == runs.size, (offsets.shape, n_gt, runs.size)
        parts = [offsets]
        if gt_polys is not None:
            xy, poly_offsets = np.ascontiguousarray(xy, np.float64).reshape(-1), np.ascontiguousarray(poly_offsets, np.int64)
            gt_polys = np.ascontiguousarray(gt_polys, np.int32)
            n_poly = poly_offsets.size - 1
            assert gt_polys.shape == (n_gt + 1,) and int(gt_polys[-1]) == n_poly and 2 * int(poly_offsets[-1]) == xy.size, \
                (gt_polys.shape, n_gt, n_poly, xy.size)
            parts += [poly_offsets, xy]                                  # the 8-byte items first: every view stays aligned
        if boxes is not None:
            boxes = np.ascontiguousarray(boxes, np.float64).reshape(-1)
            assert boxes.size == 4 * n_gt, (boxes.size, n_gt)
            at_boxes = len(parts)
            parts.append(boxes)
        if lvis_bits is not None:
            neg_bits, nex_bits = (np.ascontiguousarray(x, np.uint32).reshape(-1) for x in lvis_bits)
            assert neg_bits.size == nex_bits.size and neg_bits.size >= 1, (neg_bits.size, nex_bits.size)
            at_bits = len(parts)
            parts += [neg_bits, nex_bits]
        parts += [table.reshape(-1)] + ([gt_polys] if gt_polys is not None else []) + [runs]
        buf = self.to_device(np.concatenate([p.view(np.uint8) for p in parts]))
        at = np.concatenate(([0], np.cumsum([p.nbytes for p in parts]))).tolist()
        gt = {"n_gt": n_gt, "offsets": buf.view((n_gt + 1,), np.int64), "rows": buf.view((table.shape[0], 3), np.int32, at[-3 if gt_polys is None else -4]),
              "runs": buf.view((runs.size,), np.uint32, at[-2])}
        if gt_polys is not None:
            gt.update(n_poly=n_poly, poly_offsets=buf.view((n_poly + 1,), np.int64, at[1]), xy=buf.view((xy.size,), np.float64, at[2]),
                      gt_polys=buf.view((n_gt + 1,), np.int32, at[-3]))
        if boxes is not None:
            gt["boxes"] = buf.view((n_gt, 4), np.float64, at[at_boxes])
        if lvis_bits is not None:
            gt["neg_bits"] = buf.view((neg_bits.size,), np.uint32, at[at_bits])
            gt["not_exhaustive_bits"] = buf.view((nex_bits.size,), np.uint32, at[at_bits + 1])
        return gt

    def _gt_counts_to_device(self, gt_counts) -> dict:
        """A list of uncompressed count arrays as an `instance_gt_to_device` dict (uploaded, which waits); such a dict as it is."""
        if isinstance(gt_counts, dict):
            return gt_counts
        offs = np.concatenate(([0], np.cumsum([len(c) for c in gt_counts]))).astype(np.int64)
        runs = np.concatenate([np.asarray(c, np.uint32) for c in gt_counts]) if len(gt_counts) else np.zeros(0, np.uint32)
        return self.instance_gt_to_device(np.zeros((len(offs) - 1, 3), np.int32), runs, offs)

    def _mask_iou_inputs(self, gt_counts, iscrowd, flags):
        """-> (gt dict, n_gt, iscrowd on the device or None, flags: a fresh zeroed int32 [1] when None) of `mask_iou` / `mask_boundary_iou`."""
        gt = self._gt_counts_to_device(gt_counts)
        crowd = None if iscrowd is None else (iscrowd if isinstance(iscrowd, DeviceArray) else self.to_device(np.asarray(iscrowd, np.uint8)))
        return gt, gt["n_gt"], crowd, flags if flags is not None else self.zeros((1,), np.int32)

    def mask_iou(self, masks: DeviceArray, gt_counts, iscrowd=None, flags: Optional[DeviceArray] = None, with_counts: bool = False):
        """pycocotools' mask.iou of dense device masks [n, h, w] (float32 / uint8 / bool) against run-length masks: gt_counts = a list of
        uncompressed count arrays (uploaded here, which waits) or an `instance_gt_to_device` dict -> (iou float64 [n, n_gt] on the device,
        flags int32 [1]); with_counts adds (inter int32 [n, n_gt], area_d int64 [n], area_g int64 [n_gt]).  Temporaries uploaded here are
        freed on return by the library's synchronising free."""
        n, h, w = masks.shape
        dt = _mask_dtype(masks, "mask_iou")
        gt_counts, n_gt, crowd, flags = self._mask_iou_inputs(gt_counts, iscrowd, flags)
        iou = self.empty((n, n_gt), np.float64)
        extra = (self.empty((n, n_gt), np.int32), self.empty((n,), np.int64), self.empty((n_gt,), np.int64)) if with_counts else (None, None, None)
        check(self.lib.odise_hip_mask_iou(self.h, _p(masks), dt, n, h, w, _p(gt_counts["runs"]), _p(gt_counts["offsets"]), n_gt, _p(crowd), _p(iou),
                                          _p(extra[0]), _p(extra[1]), _p(extra[2]), _p(flags)), "mask_iou")
        return (iou, flags) + (extra if with_counts else ())

    def instance_eval(self, out_hw, table_row, scores_row, topk: int, gt: dict, num_categories: int, image: int, rows, n_rows, flags,
                      masks: Optional[DeviceArray] = None, b: int = 0, pad_hw=(0, 0), img_hw=(0, 0), iou_thresholds=None, boundary=None) -> None:
        """Enqueue COCOeval.evaluateImg of one picture (odise_hip_instance_eval): detections = the selection table_row [1 + 2 topk] /
        scores_row [topk] of image b of the last head forward, sampled from its mask logits (pad_hw / img_hw as in `instance_rle`), or the
        dense `masks` [topk, h, w] when given; gt = `instance_gt_to_device`; rows (instance_eval.ROW_DTYPE [topk]), n_rows and flags
        (int32 [1]) are device arrays or pointers.  A gt that carries polygons goes through odise_hip_instance_eval_poly.
        boundary = (rows, n_rows) or (rows, n_rows, radius): the Boundary AP task from the same pack and decode
        (odise_hip_instance_eval_boundary; radius 0 / absent = the formula); `rows` / `n_rows` may both be None then."""
        d, _thr = _inst_eval_desc("instance_eval", out_hw=out_hw, table_row=table_row, scores_row=scores_row, topk=topk, gt=gt, num_categories=num_categories,
                                  image=image, rows=rows, n_rows=n_rows, flags=flags, masks=masks, b=b, pad_hw=pad_hw, img_hw=img_hw,
                                  iou_thresholds=iou_thresholds)
        p = _inst_poly_gt(gt)
        if boundary is not None:
            check(self.lib.odise_hip_instance_eval_boundary(self.h, C.byref(d), p, None, C.byref(_boundary_task(boundary))),
                  "instance_eval_boundary")
        elif p is not None:
            check(self.lib.odise_hip_instance_eval_poly(self.h, C.byref(d), p), "instance_eval_poly")
        else:
            check(self.lib.odise_hip_instance_eval(self.h, C.byref(d)), "instance_eval")

    def instance_boxes(self, out_hw, topk: int, table_row=None, masks: Optional[DeviceArray] = None, b: int = 0, pad_hw=(0, 0), img_hw=(0, 0),
                       boxes: Optional[DeviceArray] = None) -> DeviceArray:
        """Enqueue the boxes of a picture's instance selection (odise_hip_instance_boxes: detectron2 BitMasks.get_bounding_boxes) ->
        float32 [topk, 4] XYXY on the device, rows past the count of the table zeros.  The detections are the selection table_row
        [1 + 2 topk] of image b of the last head forward, sampled from its mask logits (pad_hw / img_hw as in `instance_rle`), or the
        dense `masks` [topk, h, w] when given (table_row optional: without one every mask counts).  Host restatement:
        instance_eval.mask_boxes."""
        from ._lib import InstBoxesDesc
        d = InstBoxesDesc()
        _fill_inst_source(d, "instance_boxes", out_hw, topk, table_row, None, masks, b, pad_hw, img_hw)
        if boxes is None:
            boxes = self.empty((int(topk), 4), np.float32)
        assert boxes.dtype == np.float32 and boxes.nbytes >= 16 * int(topk), (boxes.dtype, boxes.shape)
        d.boxes = boxes.ptr
        check(self.lib.odise_hip_instance_boxes(self.h, C.byref(d)), "instance_boxes")
        return boxes

    def box_iou(self, dt_xywh, gt_xywh, iscrowd=None) -> DeviceArray:
        """pycocotools' mask.iou of boxes (odise_hip_box_iou: maskApi.c bbIou) -> float64 [n, n_gt] on the device, bit for bit
        instance_eval.box_iou.  dt_xywh [n, 4] / gt_xywh [n_gt, 4] float64 and iscrowd [n_gt]: device arrays, or host arrays, which
        are uploaded (that waits)."""
        dev = lambda a, dt: a if isinstance(a, DeviceArray) else self.to_device(np.ascontiguousarray(a, dt))
        dt, gt = dev(dt_xywh, np.float64), dev(gt_xywh, np.float64)
        assert dt.dtype == np.float64 and gt.dtype == np.float64, (dt.dtype, gt.dtype)
        n, n_gt = dt.nbytes // 32, gt.nbytes // 32
        crowd = None if iscrowd is None else dev(iscrowd, np.uint8)
        iou = self.empty((n, n_gt), np.float64)
        check(self.lib.odise_hip_box_iou(self.h, _p(dt), n, _p(gt), n_gt, _p(crowd), _p(iou)), "box_iou")
        return iou

    def instance_eval_bbox(self, out_hw, table_row, scores_row, topk: int, gt: dict, num_categories: int, image: int, bbox_rows, bbox_n_rows,
                           flags, rows=None, n_rows=None, boxes=None, masks: Optional[DeviceArray] = None, b: int = 0, pad_hw=(0, 0),
                           img_hw=(0, 0), iou_thresholds=None, boundary=None) -> None:
        """Enqueue COCOeval.evaluateImg of one picture for "bbox" (odise_hip_instance_eval_bbox) and, when `rows` / `n_rows` are given,
        for "segm" from the same pack of the detections (exactly `instance_eval`).  Arguments as in `instance_eval`; gt must carry
        "boxes" (`instance_gt_to_device(..., boxes=instance_eval.gt_boxes(annotations))`); bbox_rows / bbox_n_rows take the bbox
        task's rows; boxes (optional, float32 [topk, 4]) the detections' XYXY boxes; boundary as in `instance_eval`: the third task
        of the same call (odise_hip_instance_eval_boundary)."""
        from ._lib import InstBboxTask
        assert "boxes" in gt, "instance_eval_bbox: the ground truth carries no boxes"
        d, _thr = _inst_eval_desc("instance_eval_bbox", out_hw=out_hw, table_row=table_row, scores_row=scores_row, topk=topk, gt=gt, num_categories=num_categories,
                                  image=image, rows=rows, n_rows=n_rows, flags=flags, masks=masks, b=b, pad_hw=pad_hw, img_hw=img_hw,
                                  iou_thresholds=iou_thresholds)
        t = InstBboxTask()
        t.gt_boxes, t.rows, t.n_rows, t.boxes = gt["boxes"].ptr, _ptr(bbox_rows), _ptr(bbox_n_rows), _ptr(boxes)
        p = _inst_poly_gt(gt)
        if boundary is not None:
            check(self.lib.odise_hip_instance_eval_boundary(self.h, C.byref(d), p, C.byref(t), C.byref(_boundary_task(boundary))),
                  "instance_eval_boundary")
            return
        check(self.lib.odise_hip_instance_eval_bbox(self.h, C.byref(d), p, C.byref(t)), "instance_eval_bbox")

    def mask_boundary(self, masks: DeviceArray, radius: int = 0, out: Optional[DeviceArray] = None, with_area: bool = False):
        """The boundaries of dense device masks [n, h, w] (float32 / uint8 / bool; odise_hip_mask_boundary: mask & ~erode(mask), the
        rule of Boundary IoU) -> uint8 [n, h, w] on the device, byte for byte instance_eval.mask_boundary; radius <= 0: the formula of
        `boundary_radius`.  with_area adds the pixels of each boundary, int64 [n]."""
        n, h, w = masks.shape
        dt = _mask_dtype(masks, "mask_boundary")
        if out is None:
            out = self.empty((n, h, w), np.uint8)
        assert out.dtype == np.uint8 and out.nbytes >= n * h * w, (out.dtype, out.shape)
        area = self.empty((n,), np.int64) if with_area else None
        check(self.lib.odise_hip_mask_boundary(self.h, _p(masks), dt, n, h, w, int(radius), _p(out), _p(area)), "mask_boundary")
        return (out, area) if with_area else out

    def mask_boundary_iou(self, masks: DeviceArray, gt_counts, iscrowd=None, radius: int = 0, flags: Optional[DeviceArray] = None):
        """`mask_iou` with the Boundary IoU beside it (odise_hip_mask_boundary_iou; host restatement instance_eval.boundary_iou) ->
        (iou, mask_iou, boundary_iou, flags): float64 [n, n_gt] each on the device, iou = min(mask_iou, boundary_iou); arguments as in
        `mask_iou`."""
        n, h, w = masks.shape
        dt = _mask_dtype(masks, "mask_boundary_iou")
        gt_counts, n_gt, crowd, flags = self._mask_iou_inputs(gt_counts, iscrowd, flags)
        iou, m_iou, b_iou = (self.empty((n, n_gt), np.float64) for _ in range(3))
        check(self.lib.odise_hip_mask_boundary_iou(self.h, _p(masks), dt, n, h, w, _p(gt_counts["runs"]), _p(gt_counts["offsets"]), n_gt, _p(crowd),
                                                   int(radius), _p(iou), _p(m_iou), _p(b_iou), None, None, None, _p(flags)), "mask_boundary_iou")
        return iou, m_iou, b_iou, flags

    def lvis_eval(self, out_hw, table_row, scores_row, topk: int, gt: dict, num_categories: int, image: int, rows, n_rows, flags,
                  masks: Optional[DeviceArray] = None, b: int = 0, pad_hw=(0, 0), img_hw=(0, 0), iou_thresholds=None) -> None:
        """Enqueue LVISEval.evaluate_img of one picture (odise_hip_lvis_eval; host restatement: lvis_eval.image_rows).  Arguments as in
        `instance_eval` with topk up to 300; gt = `instance_gt_to_device(..., lvis_bits=(neg, not_exhaustive))`.  With detections from
        the mask logits the table holds (query, class) pairs and every distinct query is packed once."""
        from ._lib import LvisTask
        assert "neg_bits" in gt, "lvis_eval: the ground truth carries no category bitsets"
        assert gt["neg_bits"].shape[0] == (int(num_categories) + 31) // 32, (gt["neg_bits"].shape, num_categories)
        d, _thr = _inst_eval_desc("lvis_eval", out_hw=out_hw, table_row=table_row, scores_row=scores_row, topk=topk, gt=gt, num_categories=num_categories,
                                  image=image, rows=rows, n_rows=n_rows, flags=flags, masks=masks, b=b, pad_hw=pad_hw, img_hw=img_hw,
                                  iou_thresholds=iou_thresholds)
        t = LvisTask()
        t.neg_bits, t.not_exhaustive_bits = gt["neg_bits"].ptr, gt["not_exhaustive_bits"].ptr
        check(self.lib.odise_hip_lvis_eval(self.h, C.byref(d), _inst_poly_gt(gt), C.byref(t)), "lvis_eval")

    def lvis_accumulate(self, blocks, npig, num_categories: int, topk: int, rec_thrs=None):
        """LVISEval.accumulate on the device (odise_hip_lvis_accumulate; host restatement: lvis_eval.accumulate, which this equals byte
        for byte): `instance_accumulate` with topk up to 300 and no maxDets axis -> (precision float64 [10, R, K, 4], recall float64
        [10, K, 4])."""
        return self.instance_accumulate(blocks, npig, num_categories, topk, rec_thrs, lvis=True)

    def instance_accumulate(self, blocks, npig, num_categories: int, topk: int, rec_thrs=None, lvis: bool = False):
        """COCOeval.accumulate on the device (odise_hip_instance_accumulate; host restatement: instance_eval.accumulate, which this
        equals byte for byte).  blocks: a sequence of (rows, counts) - `rows` a DeviceArray of instance_eval.ROW_DTYPE [slots * topk],
        `counts` a DeviceArray int32 [slots], as the evaluator keeps them - or of host arrays of those shapes, which are uploaded; no two
        slots may share an `image` number.  npig int64 [K, 4] (host or device); rec_thrs: instance_eval.REC_THRS unless given.
        -> (precision float64 [10, R, K, 4, 3], recall float64 [10, K, 4, 3]) after ONE read-back, which is the only wait.  A flag raises
        `InstanceAccumulateError` (its .flags, .precision and .recall hold what the device wrote: -1 everywhere)."""
        from ._lib import InstAccumDesc, LvisAccumDesc
        from . import instance_eval as IE
        K, topk, M = int(num_categories), int(topk), 1 if lvis else 3
        thr = np.ascontiguousarray(IE.REC_THRS if rec_thrs is None else rec_thrs, np.float64).reshape(-1)
        R = thr.size
        dev = []
        for rows, counts in blocks:
            if not isinstance(rows, DeviceArray):
                rows = self.to_device(np.ascontiguousarray(rows, IE.ROW_DTYPE).reshape(-1))
            if not isinstance(counts, DeviceArray):
                counts = self.to_device(np.ascontiguousarray(counts, np.int32).reshape(-1))
            slots = int(np.prod(counts.shape, dtype=np.int64))
            assert rows.dtype == IE.ROW_DTYPE and counts.dtype == np.int32 and int(np.prod(rows.shape, dtype=np.int64)) == slots * topk, \
                (rows.shape, rows.dtype, counts.shape, counts.dtype, topk)
            dev.append((rows, counts, slots))
        nb = len(dev)
        row_ptrs = (C.c_void_p * max(nb, 1))(*[r.ptr for r, _, _ in dev])
        count_ptrs = (C.c_void_p * max(nb, 1))(*[c.ptr for _, c, _ in dev])
        slots = (C.c_int32 * max(nb, 1))(*[s for _, _, s in dev])
        if not isinstance(npig, DeviceArray):
            npig = np.ascontiguousarray(npig, np.int64)
            assert npig.shape == (K, 4), (npig.shape, K)
            # one upload: npig | rec_thrs
            up = self.to_device(np.concatenate([npig.reshape(-1).view(np.uint8), thr.view(np.uint8)]))
            npig_d, thr_d = up.view((K, 4), np.int64), up.view((R,), np.float64, K * 32)
        else:
            npig_d, thr_d = npig, self.to_device(thr)
        n_p, n_r = 10 * R * K * 4 * M, 10 * K * 4 * M
        out = self.empty((n_p + n_r + 1,), np.float64)              # precision | recall | flags: one read-back
        flags = out.view((1,), np.int32, (n_p + n_r) * 8)
        check(self.lib.odise_hip_memset(self.h, flags.ptr, 0, 8), "memset")
        d = LvisAccumDesc() if lvis else InstAccumDesc()
        d.n_blocks, d.rows, d.counts, d.slots = nb, C.addressof(row_ptrs), C.addressof(count_ptrs), C.addressof(slots)
        d.topk, d.num_categories, d.npig, d.rec_thrs, d.n_rec = topk, K, npig_d.ptr, thr_d.ptr, R
        d.precision, d.recall, d.flags = out.ptr, out.ptr + n_p * 8, flags.ptr
        if lvis:
            check(self.lib.odise_hip_lvis_accumulate(self.h, C.byref(d)), "lvis_accumulate")
        else:
            check(self.lib.odise_hip_instance_accumulate(self.h, C.byref(d)), "instance_accumulate")
        host = out.numpy()
        precision, recall = host[:n_p].reshape((10, R, K, 4) + (() if lvis else (3,))), host[n_p:n_p + n_r].reshape((10, K, 4) + (() if lvis else (3,)))
        f = int(host[n_p + n_r:].view(np.int32)[0])
        if f:
            raise InstanceAccumulateError(f, precision, recall)
        return precision, recall

    # ---- video instance segmentation AP (include/odise_hip.h odise_hip_video_eval_*; host restatement: odise_amd/video_eval.py) --------
    def video_eval_state(self, max_tracks: int = 100, max_gt: int = 1024) -> "VideoEvalState":
        """The caller-owned accumulators of one video (odise_video_eval_state), not yet zeroed: `video_eval_reset` starts a video."""
        return VideoEvalState(self, max_tracks, max_gt)

    def video_eval_reset(self, state: "VideoEvalState") -> None:
        check(self.lib.odise_hip_video_eval_reset(self.h, C.byref(state.struct)), "video_eval_reset")

    def video_eval_frame(self, state: "VideoEvalState", out_hw, topk: int, det_slot, gt: Optional[dict], gt_slot, flags, table_row=None,
                         scores_row=None, masks: Optional[DeviceArray] = None, b: int = 0, pad_hw=(0, 0), img_hw=(0, 0)) -> None:
        """Enqueue one frame (odise_hip_video_eval_frame): the detections as in `instance_eval` (dense `masks` [topk, h, w], table_row
        optional then; or the selection table_row / scores_row of image b of the last head forward), det_slot int32 [topk] = the track of
        every table index; gt = `instance_gt_to_device` of the frame's annotations (None: none) and gt_slot int32 [n_gt] their tracks;
        slots outside the state's range are skipped.  flags int32 [1]; all device arrays or pointers."""
        from ._lib import VideoFrameDesc
        d = VideoFrameDesc()
        _fill_inst_source(d, "video_eval_frame", out_hw, topk, table_row, scores_row, masks, b, pad_hw, img_hw)
        d.det_slot, d.st, d.flags = _ptr(det_slot), C.addressof(state.struct), _ptr(flags)
        p = None
        if gt is not None and gt["n_gt"]:
            d.gt_runs, d.gt_offsets, d.n_gt, d.gt_slot = gt["runs"].ptr, gt["offsets"].ptr, int(gt["n_gt"]), _ptr(gt_slot)
            p = _inst_poly_gt(gt)
            if p is not None:
                d.polys = C.addressof(p._obj)
        check(self.lib.odise_hip_video_eval_frame(self.h, C.byref(d)), "video_eval_frame")

    def video_eval_finish(self, state: "VideoEvalState", n_tracks: int, track_scores, track_category, gt_rows, n_gt: int, num_categories: int,
                          video: int, rows, n_rows, flags, iou=None, avg_area=None, iou_thresholds=None) -> None:
        """Enqueue the end of a video (odise_hip_video_eval_finish): track_scores float32 / track_category int32 [n_tracks], gt_rows int32
        [n_gt, 3] (video_eval.gt_track_rows), rows (instance_eval.ROW_DTYPE [max_tracks]) / n_rows / flags (int32 [1]) and the optional
        dumps iou float64 [n_tracks, n_gt] / avg_area float64 [n_tracks]: device arrays or pointers."""
        from ._lib import VideoFinishDesc
        from .instance_eval import IOU_THRS
        thr = np.ascontiguousarray(IOU_THRS if iou_thresholds is None else iou_thresholds, np.float64)
        assert thr.shape == (10,), thr.shape
        d = VideoFinishDesc()
        d.st, d.n_tracks, d.track_scores, d.track_category = C.addressof(state.struct), int(n_tracks), _ptr(track_scores), _ptr(track_category)
        d.gt_rows, d.n_gt, d.num_categories, d.video, d.iou_thresholds = _ptr(gt_rows), int(n_gt), int(num_categories), int(video), thr.ctypes.data
        d.rows, d.n_rows, d.flags, d.iou, d.avg_area = _ptr(rows), _ptr(n_rows), _ptr(flags), _ptr(iou), _ptr(avg_area)
        check(self.lib.odise_hip_video_eval_finish(self.h, C.byref(d)), "video_eval_finish")

    def jpeg_decode(self, data: bytes, apply_orientation: bool = True, out: Optional[DeviceArray] = None) -> DeviceArray:
        """read_image(file, "RGB") for a baseline JPEG: host Huffman decoding, IDCT / upsampling / colour conversion / EXIF transpose on
        the device -> uint8 [H,W,3], bit-identical to Pillow.  Baseline, extended-sequential and progressive files; raises `UnsupportedInput` for arithmetic-coded / CMYK / RGB-coded ones."""
        info = jpeg_info(data)
        swap = apply_orientation and info["orientation"] >= 5
        oh, ow = (info["width"], info["height"]) if swap else (info["height"], info["width"])
        if out is None or out.nbytes < oh * ow * 3:
            out = self.empty((oh, ow, 3), np.uint8)
        h, w = C.c_int(0), C.c_int(0)
        buf = (C.c_ubyte * len(data)).from_buffer_copy(data)
        check(self.lib.odise_hip_jpeg_decode(self.h, buf, C.c_int64(len(data)), _p(out), C.c_int64(out.nbytes), int(bool(apply_orientation)),
                                             C.byref(h), C.byref(w)), "jpeg_decode")
        return out.view((h.value, w.value, 3)) if out.shape != (h.value, w.value, 3) else out


class VideoEvalState:
    """odise_video_eval_state: the sums of one video in ONE device buffer - inter int64 [max_tracks, max_gt] | area_d int64 [max_tracks] |
    area_g int64 [max_gt] | frames_d int32 [max_tracks] - with `.struct` for the calls.  `numpy()` reads all four back at once."""

    def __init__(self, ctx: "Context", max_tracks: int, max_gt: int):
        from ._lib import VideoEvalState as _State
        self.ctx, self.max_tracks, self.max_gt = ctx, int(max_tracks), int(max_gt)
        T, G = self.max_tracks, self.max_gt
        self.buf = ctx.empty((8 * (T * G + T + G) + 4 * T,), np.uint8)
        self.inter = self.buf.view((T, G), np.int64)
        self.area_d = self.buf.view((T,), np.int64, 8 * T * G)
        self.area_g = self.buf.view((G,), np.int64, 8 * (T * G + T))
        self.frames_d = self.buf.view((T,), np.int32, 8 * (T * G + T + G))
        self.struct = _State()
        self.struct.inter, self.struct.area_d, self.struct.area_g, self.struct.frames_d = self.inter.ptr, self.area_d.ptr, self.area_g.ptr, self.frames_d.ptr
        self.struct.max_tracks, self.struct.max_gt = T, G

    def numpy(self):
        """-> (inter, area_d, area_g, frames_d) on the host (one read, which waits)."""
        T, G = self.max_tracks, self.max_gt
        raw = self.buf.numpy()
        i64 = raw[:8 * (T * G + T + G)].view(np.int64)
        return i64[:T * G].reshape(T, G), i64[T * G:T * G + T], i64[T * G + T:], raw[8 * (T * G + T + G):].view(np.int32)

    def copy_from(self, inter, area_d, area_g, frames_d) -> None:
        """Upload all four (tests preload them)."""
        parts = [np.ascontiguousarray(inter, np.int64).reshape(-1), np.ascontiguousarray(area_d, np.int64), np.ascontiguousarray(area_g, np.int64),
                 np.ascontiguousarray(frames_d, np.int32)]
        self.buf.copy_from(np.concatenate([p.view(np.uint8) for p in parts]))


class _Handle:
    """An object of the library behind a handle.  A subclass sets `ctx` and calls `_create`; its class attributes `_reset` and `_destroy`
    name the library's functions (without the odise_hip_ prefix).  `close()` (or collection) releases it."""
    _reset = _destroy = ""
    handle = None

    def _create(self, name: str, *args) -> None:
        h = C.c_void_p()
        check(getattr(self.ctx.lib, "odise_hip_" + name)(self.ctx.h, *args, C.byref(h)), name)
        self.handle = h.value

    def reset(self) -> None:
        check(getattr(self.ctx.lib, "odise_hip_" + self._reset)(self.ctx.h, C.c_void_p(self.handle)), self._reset)

    def close(self) -> None:
        if self.handle and self.ctx.h:
            getattr(self.ctx.lib, "odise_hip_" + self._destroy)(self.ctx.h, C.c_void_p(self.handle))
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _track_pool(pool) -> np.ndarray:
    """The colour pool of a tracker, uint8 [P,3] on the host: video.default_pool() when None."""
    from .video import default_pool
    return default_pool() if pool is None else np.ascontiguousarray(np.asarray(pool, np.uint8).reshape(-1, 3))


class Tracker(_Handle):
    """odise_track (include/odise_hip.h): the library's tracker object for frames of one size; `close()` (or collection) releases it."""
    _reset, _destroy = "track_reset", "track_destroy"

    def __init__(self, ctx: Context, hw, ttl: int = 8, pool=None):
        self.ctx, self.hw, self.ttl, self.pool = ctx, (int(hw[0]), int(hw[1])), int(ttl), _track_pool(pool)
        self._create("track_create", self.hw[0], self.hw[1], self.ttl, self.pool.ctypes.data_as(C.c_void_p), len(self.pool))


class InstTracker(_Handle):
    """odise_inst_track (include/odise_hip.h): the library's tracker object for selections of `topk` instance masks of one size;
    `close()` (or collection) releases it."""
    _reset, _destroy = "inst_track_reset", "inst_track_destroy"

    def __init__(self, ctx: Context, hw, topk: int, ttl: int = 8, pool=None):
        self.ctx, self.hw, self.topk, self.ttl, self.pool = ctx, (int(hw[0]), int(hw[1])), int(topk), int(ttl), _track_pool(pool)
        self._create("inst_track_create", self.hw[0], self.hw[1], self.topk, self.ttl, self.pool.ctypes.data_as(C.c_void_p), len(self.pool))


class BoxTracker(_Handle):
    """odise_box_track (include/odise_hip.h): the library's tracker object for selections of `topk` instance boxes; `close()` (or
    collection) releases it."""
    _reset, _destroy = "box_track_reset", "box_track_destroy"

    def __init__(self, ctx: Context, topk: int, ttl: int = 8, pool=None):
        self.ctx, self.topk, self.ttl, self.pool = ctx, int(topk), int(ttl), _track_pool(pool)
        self._create("box_track_create", self.topk, self.ttl, self.pool.ctypes.data_as(C.c_void_p), len(self.pool))


class SemanticTTA(_Handle):
    """odise_tta (include/odise_hip.h): the views of one picture laid end to end for one semantic product; `close()` (or collection)
    releases the device buffers (S_cat: out_h * out_w * max_views * Qpad fp16)."""
    _reset, _destroy = "tta_reset", "tta_destroy"

    def __init__(self, ctx: Context, out_hw, K: int, Q: int, max_views: int):
        self.ctx, self.hw, self.K, self.Q, self.max_views = ctx, (int(out_hw[0]), int(out_hw[1])), int(K), int(Q), int(max_views)
        self._create("tta_create", self.hw[0], self.hw[1], self.K, self.Q, self.max_views)

    def add_view(self, b: int, mask_cls_b, pad_hw, img_hw, hflip: bool = False) -> None:
        """Image b of the context's current mask logits + its log-probabilities (DeviceArray fp32 [Q, K+1], or a device pointer)."""
        check(self.ctx.lib.odise_hip_tta_add_view(self.ctx.h, C.c_void_p(self.handle), int(b), mask_cls_b, int(pad_hw[0]), int(pad_hw[1]),
                                                  int(img_hw[0]), int(img_hw[1]), int(bool(hflip))), "tta_add_view")

    def finish(self, sem_seg: Optional[DeviceArray] = None, sem_argmax: Optional[DeviceArray] = None) -> None:
        """sem_seg fp32 [K,H,W] = mean over the views; sem_argmax int32 [H,W] = first maximum of their sum.  Either or both."""
        check(self.ctx.lib.odise_hip_tta_finish(self.ctx.h, C.c_void_p(self.handle), _p(sem_seg), _p(sem_argmax)), "tta_finish")


class RlePending:
    """An enqueued RLE call.  `result()` reads the offsets back (one synchronisation); when the strings did not fit (offsets[n] > capacity,
    nothing written) it enqueues the call once more with exactly offsets[n] bytes, then reads the strings.  `bufs` = (bytes, offsets, area)
    device arrays to use instead of fresh ones (uint8 [capacity], int64 [n + 1], int64 [n]); `grow(nbytes) -> DeviceArray` provides the
    buffer of the retry (a caller's pool; default: a new device array)."""

    def __init__(self, ctx: Context, n: int, size, launch, capacity: Optional[int] = None, bufs=None, trim: bool = False, grow=None):
        self.ctx, self.n, self.size, self.launch, self.trim = ctx, int(n), [int(size[0]), int(size[1])], launch, trim
        self.grow = grow if grow is not None else (lambda nbytes: ctx.empty((nbytes,), np.uint8))
        if bufs is None:
            cap = int(capacity) if capacity is not None else Context.RLE_BYTES_PER_MASK * max(self.n, 1)
            bufs = (ctx.empty((max(cap, 1),), np.uint8), ctx.empty((self.n + 1,), np.int64), ctx.empty((max(self.n, 1),), np.int64))
        self.buf, self.off, self.area = bufs
        self.capacity = self.buf.nbytes if capacity is None else int(capacity)
        assert 0 <= self.capacity <= self.buf.nbytes and self.off.nbytes >= 8 * (self.n + 1) and self.area.nbytes >= 8 * self.n
        launch(self.buf, self.capacity, self.off, self.area)

    def result(self):
        off = self.off.view((self.n + 1,), np.int64).numpy()
        total = int(off[-1])
        buf = self.buf
        if total > self.capacity:                                       # nothing was written: once more with the exact size
            buf = self.grow(total)
            assert buf.nbytes >= total, (buf.nbytes, total)
            self.launch(buf, total, self.off, self.area)
            off = self.off.view((self.n + 1,), np.int64).numpy()
            assert int(off[-1]) == total, (int(off[-1]), total)
        raw = buf.view((total,), np.uint8).numpy().tobytes() if total else b""
        area = self.area.view((self.n,), np.int64).numpy() if self.n else np.zeros((0,), np.int64)
        rles = [{"size": list(self.size), "counts": raw[off[i]:off[i + 1]].decode("ascii")} for i in range(self.n)]
        if self.trim:                                                   # instance selections: entries past the device-side count are empty
            k = int(np.count_nonzero(np.diff(off)))
            rles, area = rles[:k], area[:k]
        return rles, area


class SemSegPending:
    """An enqueued `odise_hip_semantic_eval` call (with `pq_stats`: `odise_hip_semantic_eval_pq`, the first launch and only the first).
    The matrices and the PQ statistics are counted by the first launch only, and the ground truth is let go of right after it.  `settle()` reads n_classes and the offsets back (one synchronisation) and enqueues the RLE part again -
    without the counters - at most twice: with max_classes = n_classes when more classes are present than were asked for, and with
    exactly offsets[-1] bytes when the strings did not fit.  A retry READS `pred` AGAIN (from a score tensor it takes the whole K-plane
    arg-max again, about the cost of the first call: the labels of the first launch lay in the context's shared scratch and are gone), so
    `settle()` must run while `pred` still holds the picture; after it `pred` is let go of and `result()` reads only buffers of this
    object.  `result()` settles first when nobody has: then the caller keeps `pred` untouched until `result()`."""

    def __init__(self, ctx: Context, pred, K, hw, gt, conf, b_conf, flags, radius, rle, max_classes, capacity, bufs=None, pq_stats=None):
        from ._lib import MAX_SEGMENTS
        self.ctx, self.pred, self.K, self.hw, self.conf, self.b_conf, self.flags, self.radius = ctx, pred, K, hw, conf, b_conf, flags, radius
        self.pq_stats = pq_stats
        self.rle = rle
        self.max_classes = int(max_classes) if max_classes is not None else MAX_SEGMENTS
        self.capacity = int(capacity) if capacity is not None else Context.sem_rle_bytes(hw)
        self.launches = 0
        self._settled = None
        if rle and bufs is not None:
            self.buf, self.meta, self.off = bufs
            assert self.buf.nbytes >= self.capacity and self.meta.nbytes >= 4 * (1 + self.max_classes) and self.off.nbytes >= 8 * (2 * self.max_classes + 1)
        elif rle:
            self._alloc()
        counting = gt is not None and (conf is not None or b_conf is not None or pq_stats is not None)
        self._launch(gt if counting else None)
        if not rle:
            self.pred = None

    def _alloc(self):
        n = self.max_classes
        self.buf = self.ctx.empty((max(self.capacity, 1),), np.uint8)
        self.meta = self.ctx.empty((1 + n,), np.int32)              # n_classes | classes
        self.off = self.ctx.empty((2 * n + 1,), np.int64)           # offsets [n + 1] | area [n]

    def _launch(self, gt=None):
        """gt None: the strings alone (a retry)."""
        from ._lib import SemSegEvalDesc
        d = SemSegEvalDesc()
        d.K, d.H, d.W, d.radius = self.K, self.hw[0], self.hw[1], self.radius
        if self.pred.dtype == np.float32:
            d.sem_seg = self.pred.ptr
        else:
            d.labels = self.pred.ptr
        d.flags = self.flags.ptr
        if gt is not None:
            d.gt = gt.ptr
            d.conf = self.conf.ptr if self.conf is not None else None
            d.b_conf = self.b_conf.ptr if self.b_conf is not None else None
        if self.rle:
            n = self.max_classes
            d.max_classes, d.n_classes, d.classes = n, self.meta.ptr, self.meta.ptr + 4
            d.rle, d.capacity, d.offsets, d.area = self.buf.ptr, self.capacity, self.off.ptr, self.off.ptr + 8 * (n + 1)
        if gt is not None and self.pq_stats is not None:
            from ._lib import SemSegPqTask
            t = SemSegPqTask()
            t.stats = self.pq_stats.ptr
            check(self.ctx.lib.odise_hip_semantic_eval_pq(self.ctx.h, C.byref(d), C.byref(t)), "semantic_eval_pq")
        else:
            check(self.ctx.lib.odise_hip_semantic_eval(self.ctx.h, C.byref(d)), "semantic_eval")
        self.launches += 1

    def settle(self) -> "SemSegPending":
        """Read n_classes and the offsets, enqueue the retries the picture needs (they read `pred`), let go of `pred`."""
        if self._settled is not None or not self.rle:
            return self
        meta = self.meta.view((1 + self.max_classes,), np.int32).numpy()
        if int(meta[0]) > self.max_classes:                           # more classes present than asked for: once more for all of them
            self.max_classes = int(meta[0])
            self._alloc()
            self._launch()
            meta = self.meta.numpy()
        n = int(meta[0])
        assert n <= self.max_classes, (n, self.max_classes)
        off = self.off.view((2 * self.max_classes + 1,), np.int64).numpy()
        total = int(off[self.max_classes])
        if total > self.capacity:                                     # nothing was written: once more with the exact size
            self.capacity = total
            self.buf = self.ctx.empty((total,), np.uint8)
            self._launch()
            off = self.off.numpy()
            assert int(off[self.max_classes]) == total, (int(off[self.max_classes]), total)
        self._settled = (meta[1:1 + n].copy(), off[:n + 1].copy(), off[self.max_classes + 1:self.max_classes + 1 + n].copy())
        self.pred = self.meta = self.off = None                       # the strings in self.buf are all that is still to be read
        return self

    def result(self):
        if not self.rle:
            return np.zeros(0, np.int32), [], np.zeros(0, np.int64)
        classes, off, area = self.settle()._settled
        total = int(off[-1])
        raw = self.buf.view((total,), np.uint8).numpy().tobytes() if total else b""
        rles = [{"size": [int(self.hw[0]), int(self.hw[1])], "counts": raw[off[i]:off[i + 1]].decode("ascii")} for i in range(len(classes))]
        return classes, rles, area


def _jpeg_info_struct(info: dict):
    from ._lib import JpegInfo
    st = JpegInfo()
    for k in ("width", "height", "components", "h_samp", "v_samp", "orientation", "restart_interval", "coef_count"):
        setattr(st, k, info[k])
    for c in range(info["components"]):
        st.blocks_x[c], st.blocks_y[c] = info["blocks_x"][c], info["blocks_y"][c]
    return st


def jpeg_decode_coefs(ctx: Context, info: dict, coefs, qt, apply_orientation: bool = True) -> DeviceArray:
    """Device half of the decoder on coefficients from `jpeg_entropy_decode` (which may have run in a loader thread)."""
    swap = apply_orientation and info["orientation"] >= 5
    oh, ow = (info["width"], info["height"]) if swap else (info["height"], info["width"])
    out = ctx.empty((oh, ow, 3), np.uint8)
    flat = coefs if isinstance(coefs, np.ndarray) else np.concatenate([np.asarray(c).ravel() for c in coefs])
    flat = np.ascontiguousarray(flat.ravel(), np.int16)
    qt = np.ascontiguousarray(qt, np.uint16)
    st = _jpeg_info_struct(info)
    check(ctx.lib.odise_hip_jpeg_decode_coefs(ctx.h, C.byref(st), flat.ctypes.data_as(C.c_void_p), qt.ctypes.data_as(C.c_void_p), _p(out),
                                              C.c_int64(out.nbytes), int(bool(apply_orientation)), None, None), "jpeg_decode_coefs")
    return out


def jpeg_info(data: bytes) -> dict:
    """Header fields of a JPEG byte stream (host only)."""
    from ._lib import JpegInfo, load
    info = JpegInfo()
    buf = (C.c_ubyte * len(data)).from_buffer_copy(data)
    check(load().odise_hip_jpeg_info(buf, C.c_int64(len(data)), C.byref(info)), "jpeg_info")
    return dict(width=info.width, height=info.height, components=info.components, h_samp=info.h_samp, v_samp=info.v_samp,
                orientation=info.orientation, restart_interval=info.restart_interval, blocks_x=list(info.blocks_x)[:info.components],
                blocks_y=list(info.blocks_y)[:info.components], coef_count=info.coef_count)


def jpeg_entropy_decode(data: bytes, flat: bool = False):
    """Host half of the decoder on its own: (info, [int16 [blocks_y, blocks_x, 64] per component], uint16 [components, 64] tables);
    `flat=True` returns the coefficients as the one int16 array `jpeg_decode_coefs` uploads.  Thread-safe (no context involved)."""
    from ._lib import load
    info = jpeg_info(data)
    coefs = np.zeros(info["coef_count"], np.int16)
    qt = np.zeros((info["components"], 64), np.uint16)
    buf = (C.c_ubyte * len(data)).from_buffer_copy(data)
    check(load().odise_hip_jpeg_entropy_decode(buf, C.c_int64(len(data)), coefs.ctypes.data_as(C.c_void_p), C.c_int64(coefs.size),
                                               qt.ctypes.data_as(C.c_void_p)), "jpeg_entropy_decode")
    if flat:
        return info, coefs, qt
    out, off = [], 0
    for by, bx in zip(info["blocks_y"], info["blocks_x"]):
        out.append(coefs[off:off + by * bx * 64].reshape(by, bx, 64))    # views of one flat array (what jpeg_decode_coefs uploads)
        off += by * bx * 64
    return info, out, qt


_default: Optional[Context] = None


def default_context() -> Context:
    """Process-wide context on cuda:<LOCAL_RANK> (one process per GPU)."""
    global _default
    if _default is None:
        import os
        _default = Context(int(os.environ.get("LOCAL_RANK", "0")))
    return _default
