// rgb.h — packed RGB bytes as the drawing, quality and tracking kernels move them (vis.hip, vis_inst.hip, pq.hip, track.hip): a pixel is
// r | g << 8 | b << 16, four pixels travel as three dwords where their 12 bytes are 4-byte aligned, and the alpha blend of a pixel.
#pragma once
#include "common.h"

namespace odise {

__device__ __forceinline__ void rgb4_unpack(unsigned d0, unsigned d1, unsigned d2, unsigned px[4]) {
    px[0] = d0 & 0xffffffu; px[1] = (d0 >> 24) | ((d1 & 0xffffu) << 8); px[2] = (d1 >> 16) | ((d2 & 0xffu) << 16); px[3] = d2 >> 8;
}
__device__ __forceinline__ void rgb4_pack(const unsigned px[4], unsigned d[3]) {   // d may be the picture itself
    d[0] = px[0] | (px[1] << 24); d[1] = (px[1] >> 8) | (px[2] << 16); d[2] = (px[2] >> 16) | (px[3] << 8);
}
__device__ __forceinline__ unsigned rgb_load(const uint8_t* p) { return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16); }
__device__ __forceinline__ void rgb_store(uint8_t* p, unsigned v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); }

// (v * (256 - a) + c * a + 128) >> 8 per channel, with the colour's share worked out once per colour: crb holds it for red and blue, cg for green
__device__ __forceinline__ void blend_color(unsigned c, unsigned alpha, unsigned& crb, unsigned& cg) {
    crb = (c & 0xff00ffu) * alpha + 0x800080u;
    cg = ((c >> 8) & 0xffu) * alpha + 128u;
}
__device__ __forceinline__ unsigned blend_rgb(unsigned v, unsigned ia, unsigned crb, unsigned cg) {   // ia = 256 - alpha
    // red and blue in one multiply: a channel's v * ia + c * a + 128 <= 255 * 256 + 128 stays inside its 16 bits
    const unsigned rb = (((v & 0xff00ffu) * ia + crb) >> 8) & 0xff00ffu;
    const unsigned g = (((v >> 8) & 0xffu) * ia + cg) >> 8;
    return rb | (g << 8);
}

}  // namespace odise
