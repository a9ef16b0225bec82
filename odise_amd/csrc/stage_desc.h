// stage_desc.h — the GEMM / attention descriptors of the model stages (unet.cpp, extractor.cpp, maskgen.cpp, classify.cpp), built in one
// place.  Plain functions of shapes and pointers: no HIP calls, nothing but the C ABI's structs, so tests/test_stage_desc_cpu.py can compare
// every builder with a descriptor written out by hand.  Every field a builder does not name is zero.
#pragma once
#include <math.h>

#include "../../include/odise_hip.h"

namespace odise {

// y[M, out] = act(x[M, in] W^T + b) (+ residual [M, ldc]); geglu: y[M, out / 2].  w: anything with (w, b, in, out) - engine.h LinW
template <class Lin>
inline odise_gemm_desc gemm_linear(const void* x, int64_t M, const Lin& w, void* y, int c_dtype = ODISE_F16, int act = ODISE_ACT_NONE,
                                   const void* residual = nullptr, bool geglu = false) {
    odise_gemm_desc d = {};
    d.M = (int)M; d.N = w.out; d.K = w.in;
    d.A = x; d.lda = w.in;
    d.W = w.w; d.ldw = w.in;
    d.C = y; d.ldc = geglu ? w.out / 2 : w.out; d.c_dtype = c_dtype;
    d.bias_n = w.b;
    d.residual = residual; d.ldr = d.ldc;
    d.act = act; d.geglu = geglu ? 1 : 0; d.alpha = 1.f; d.batch = 1;
    return d;
}

// V^T = Wv x^T + bias_m (the bias runs along the rows) -> [out, ldvt]: the weight is the A operand, the `cols` token rows of x the W operand.
// One GEMM; with cols = images x tokens-per-image every image's V^T is a column block of the same matrix (attention: strideVt = tokens-per-image)
template <class Lin>
inline odise_gemm_desc gemm_vt(const Lin& v, const float* bias_m, const void* x, int64_t cols, int64_t ldvt, void* vt) {
    odise_gemm_desc d = {};
    d.M = v.out; d.N = (int)cols; d.K = v.in;
    d.A = v.w; d.lda = v.in;
    d.W = x; d.ldw = v.in;
    d.C = vt; d.ldc = ldvt; d.c_dtype = ODISE_F16;
    d.bias_m = bias_m; d.alpha = 1.f; d.batch = 1;
    return d;
}

// V^T[b] = Wv x[b]^T + bias_m -> [B, out, ldvt]: x [B, L, in] packed, one matrix per image (attention: strideVt = out * ldvt)
template <class Lin>
inline odise_gemm_desc gemm_vt(const Lin& v, const float* bias_m, const void* x, int B, int64_t L, int64_t ldvt, void* vt) {
    odise_gemm_desc d = gemm_vt(v, bias_m, x, L, ldvt, vt);
    d.strideW = L * v.in; d.strideC = (int64_t)v.out * ldvt; d.batch = B;
    return d;
}

// C[b] = alpha * A[b] (M x K) W[b]^T (N x K), element strides between the matrices of a batch
inline odise_gemm_desc gemm_batched_nt(const void* A, int64_t lda, int64_t strideA, const void* W, int64_t ldw, int64_t strideW, void* C, int64_t ldc,
                                       int64_t strideC, int64_t M, int64_t N, int64_t K, int batch, int c_dtype = ODISE_F16, float alpha = 1.f) {
    odise_gemm_desc d = {};
    d.M = (int)M; d.N = (int)N; d.K = (int)K;
    d.A = A; d.lda = lda; d.strideA = strideA;
    d.W = W; d.ldw = ldw; d.strideW = strideW;
    d.C = C; d.ldc = ldc; d.strideC = strideC; d.c_dtype = c_dtype;
    d.alpha = alpha; d.batch = batch;
    return d;
}

// softmax(scale * Q K^T + mask) V over B x H (image, head) pairs; scale = 1 / sqrt(D) unless set afterwards.  Operands: (pointer, row stride,
// element stride between images); all fp16 but the u8 mask.
struct attn_desc : odise_attn_desc {
    attn_desc(int B_, int H_, int64_t Lq_, int64_t Lk_, int D_) : odise_attn_desc{} {
        B = B_; H = H_; Lq = (int)Lq_; Lk = (int)Lk_; D = D_;
        scale = 1.0f / sqrtf((float)D_);
    }
    attn_desc& q(const void* p, int64_t ld, int64_t stride) { Q = p; ldq = ld; strideQ = stride; return *this; }
    attn_desc& k(const void* p, int64_t ld, int64_t stride) { K = p; ldk = ld; strideK = stride; return *this; }
    attn_desc& vt(const void* p, int64_t ld, int64_t stride) { Vt = p; ldvt = ld; strideVt = stride; return *this; }
    attn_desc& o(void* p, int64_t ld, int64_t stride) { O = p; ldo = ld; strideO = stride; return *this; }
    // the output of a fused q|k projection: rows of ld = 2 x width elements, q in the first half and k in the second
    attn_desc& qk_fused(const void* buf, int64_t ld, int64_t stride) { return q(buf, ld, stride).k((const uint16_t*)buf + ld / 2, ld, stride); }
    attn_desc& mask(const uint8_t* p, int64_t ld, int64_t stride) { odise_attn_desc::mask = p; ldmask = ld; strideMask = stride; return *this; }
};

}  // namespace odise
