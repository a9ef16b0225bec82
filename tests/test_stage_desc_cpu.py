"""The stage code's descriptor builders (odise_amd/csrc/stage_desc.h) against descriptors written out by hand, field by field, at the smallest
shapes where the padding and stride rules differ from the packed ones.  A stand-alone host program (its own main, only stage_desc.h and
odise_hip.h) built with AddressSanitizer + UBSan and run directly: no GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <stdio.h>
#include <string.h>

#include "stage_desc.h"

using namespace odise;

struct Lin { const uint16_t* w; const float* b; int in, out; };   // the (w, b, in, out) of engine.h LinW

static int bad = 0;
#define EQ(f) do { if (!(got.f == want.f)) { printf("%s: field %s differs\n", name, #f); ++bad; } } while (0)

static void same(const char* name, const odise_gemm_desc& got, const odise_gemm_desc& want) {
    EQ(M); EQ(N); EQ(K); EQ(A); EQ(lda); EQ(W); EQ(ldw); EQ(C); EQ(ldc); EQ(c_dtype); EQ(bias_n); EQ(bias_m); EQ(scale_m); EQ(residual); EQ(ldr);
    EQ(rowgroup_add); EQ(rows_per_group); EQ(ldg); EQ(act); EQ(geglu); EQ(alpha); EQ(batch); EQ(strideA); EQ(strideW); EQ(strideC); EQ(strideR);
}
static void same(const char* name, const odise_attn_desc& got, const odise_attn_desc& want) {
    EQ(B); EQ(H); EQ(Lq); EQ(Lk); EQ(D); EQ(Q); EQ(ldq); EQ(strideQ); EQ(K); EQ(ldk); EQ(strideK); EQ(Vt); EQ(ldvt); EQ(strideVt);
    EQ(O); EQ(ldo); EQ(strideO); EQ(mask); EQ(ldmask); EQ(strideMask); EQ(scale);
}

int main() {
    // never dereferenced: distinct addresses are all the builders need
    static uint16_t wbuf[8], xbuf[8], ybuf[8], qbuf[4096], kbuf[8], vbuf[8], obuf[8], rbuf[8];
    static float bias[8], fout[8];
    static uint8_t mbuf[8];
    odise_gemm_desc g;
    odise_attn_desc a;

    {   // V^T of the 77 context tokens: 80 columns per row, three images, no bias
        const Lin v{wbuf, nullptr, 768, 320};
        memset(&g, 0, sizeof g);
        g.M = 320; g.N = 77; g.K = 768;
        g.A = wbuf; g.lda = 768; g.strideA = 0;
        g.W = xbuf; g.ldw = 768; g.strideW = 77 * 768;
        g.C = ybuf; g.ldc = 80; g.strideC = 320 * 80; g.c_dtype = ODISE_F16;
        g.alpha = 1.f; g.batch = 3;
        same("vt L=77 ldvt=80", gemm_vt(v, nullptr, xbuf, 3, 77, 80, ybuf), g);
    }
    {   // V^T of 100 tokens in rows of 104, two images, the bias along the rows
        const Lin v{wbuf, nullptr, 256, 256};
        memset(&g, 0, sizeof g);
        g.M = 256; g.N = 100; g.K = 256;
        g.A = wbuf; g.lda = 256;
        g.W = xbuf; g.ldw = 256; g.strideW = 100 * 256;
        g.C = ybuf; g.ldc = 104; g.strideC = 256 * 104; g.c_dtype = ODISE_F16;
        g.bias_m = bias; g.alpha = 1.f; g.batch = 2;
        same("vt L=100 ldvt=104 B=2", gemm_vt(v, bias, xbuf, 2, 100, 104, ybuf), g);
    }
    {   // attention over a fused q|k buffer: C = 64, 8 heads of 8, 9 tokens; V^T rows of 16
        memset(&a, 0, sizeof a);
        a.B = 2; a.H = 8; a.Lq = 9; a.Lk = 9; a.D = 8;
        a.Q = qbuf; a.ldq = 128; a.strideQ = 9 * 128;
        a.K = qbuf + 64; a.ldk = 128; a.strideK = 9 * 128;
        a.Vt = vbuf; a.ldvt = 16; a.strideVt = 64 * 16;
        a.O = obuf; a.ldo = 64; a.strideO = 9 * 64;
        a.scale = 1.0f / sqrtf(8.0f);
        same("attn fused q|k", attn_desc(2, 8, 9, 9, 8).qk_fused(qbuf, 128, 9 * 128).vt(vbuf, 16, 64 * 16).o(obuf, 64, 9 * 64), a);
    }
    {   // attention against precomputed K / V^T: 5 queries, 77 keys, mask rows of 80 taken out of a [577 + 5][80] block per image
        memset(&a, 0, sizeof a);
        a.B = 2; a.H = 16; a.Lq = 5; a.Lk = 77; a.D = 64;
        a.Q = qbuf; a.ldq = 1024; a.strideQ = 5 * 1024;
        a.K = kbuf; a.ldk = 1024; a.strideK = 77 * 1024;
        a.Vt = vbuf; a.ldvt = 80; a.strideVt = 1024 * 80;
        a.O = obuf; a.ldo = 1024; a.strideO = 5 * 1024;
        a.mask = mbuf; a.ldmask = 80; a.strideMask = (577 + 5) * 80;
        a.scale = 0.125f;
        same("attn precomputed K / V^T + mask", attn_desc(2, 16, 5, 77, 64).q(qbuf, 1024, 5 * 1024).k(kbuf, 1024, 77 * 1024).vt(vbuf, 80, 1024 * 80)
                 .o(obuf, 1024, 5 * 1024).mask(mbuf, 80, (577 + 5) * 80), a);
    }
    {   // V^T of two images of TP = 584 token rows side by side: ONE GEMM, ldc = the store's row length, no batch strides
        const Lin v{wbuf, nullptr, 1024, 1024};
        memset(&g, 0, sizeof g);
        g.M = 1024; g.N = 2 * 584; g.K = 1024;
        g.A = wbuf; g.lda = 1024;
        g.W = xbuf; g.ldw = 1024;
        g.C = ybuf; g.ldc = 3504; g.c_dtype = ODISE_F16;
        g.bias_m = bias; g.alpha = 1.f; g.batch = 1;
        same("vt side by side TP=584 B=2", gemm_vt(v, bias, xbuf, 2 * 584, 3504, ybuf), g);
        // ... which the attention reads with strideVt = TP
        memset(&a, 0, sizeof a);
        a.B = 2; a.H = 16; a.Lq = 577; a.Lk = 577; a.D = 64;
        a.Q = qbuf; a.ldq = 2048; a.strideQ = 584 * 2048;
        a.K = qbuf + 1024; a.ldk = 2048; a.strideK = 584 * 2048;
        a.Vt = ybuf; a.ldvt = 3504; a.strideVt = 584;
        a.O = obuf; a.ldo = 1024; a.strideO = 584 * 1024;
        a.scale = 0.125f;
        same("attn side by side", attn_desc(2, 16, 577, 577, 64).qk_fused(qbuf, 2048, 584 * 2048).vt(ybuf, 3504, 584).o(obuf, 1024, 584 * 1024), a);
    }
    {   // GEGLU linear: 2560 interleaved (a, gate) columns -> 1280 outputs; the residual has the output's row length
        const Lin w{wbuf, bias, 320, 2560};
        memset(&g, 0, sizeof g);
        g.M = 37; g.N = 2560; g.K = 320;
        g.A = xbuf; g.lda = 320; g.W = wbuf; g.ldw = 320;
        g.C = ybuf; g.ldc = 1280; g.c_dtype = ODISE_F16;
        g.bias_n = bias; g.residual = rbuf; g.ldr = 1280;
        g.act = ODISE_ACT_NONE; g.geglu = 1; g.alpha = 1.f; g.batch = 1;
        same("linear geglu", gemm_linear(xbuf, 37, w, ybuf, ODISE_F16, ODISE_ACT_NONE, rbuf, true), g);
    }
    {   // plain linear with fp32 output
        const Lin w{wbuf, bias, 256, 24};
        memset(&g, 0, sizeof g);
        g.M = 200; g.N = 24; g.K = 256;
        g.A = xbuf; g.lda = 256; g.W = wbuf; g.ldw = 256;
        g.C = fout; g.ldc = 24; g.c_dtype = ODISE_F32; g.ldr = 24;
        g.bias_n = bias; g.alpha = 1.f; g.batch = 1;
        same("linear f32 out", gemm_linear(xbuf, 200, w, fout, ODISE_F32), g);
    }
    {   // batched A[b] W[b]^T with explicit strides: q k^T of a fused q|k buffer into rows of 72, scaled
        memset(&g, 0, sizeof g);
        g.M = 65; g.N = 65; g.K = 32;
        g.A = qbuf; g.lda = 64; g.strideA = 65 * 64;
        g.W = qbuf + 32; g.ldw = 64; g.strideW = 65 * 64;
        g.C = ybuf; g.ldc = 72; g.strideC = 65 * 72; g.c_dtype = ODISE_F16;
        g.alpha = 0.25f; g.batch = 2;
        same("batched nt", gemm_batched_nt(qbuf, 64, 65 * 64, qbuf + 32, 64, 65 * 64, ybuf, 72, 65 * 72, 65, 65, 32, 2, ODISE_F16, 0.25f), g);
    }
    if (bad) return 1;
    printf("ok\n");
    return 0;
}
"""


def test_builders_equal_hand_written_descriptors(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is required to build the host check"
    src, exe = tmp_path / "stage_desc_check.cpp", tmp_path / "stage_desc_check"
    src.write_text(PROGRAM)
    cmd = [cxx, "-std=c++17", "-O0", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "odise_amd", "csrc"), str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
