// The launchers behind the C ABI: one prototype per kernel family, shared by the files that call across (conv.hip, plan.hip,
// stem012.hip, wgrad.hip).  The conv launchers take a segment of a route (conv_route.h) and only launch it.
#pragma once
#include "common.h"
#include "conv_route.h"

namespace ppnconv {
int launch_big(const ConvSegment& s, hipStream_t st);                                         // conv_big.hip
}

namespace ppn {
// conv.hip: route the descriptor, write *stats_tiles, launch each segment.  kname: the first segment's kernel name; strip: whether
// the last 16-bit large-tile segment took the strip loader
int conv_launch(const ppn_conv_desc* d, hipStream_t st, const char** kname, int* strip = nullptr);
int split_x3_launch(const float* src, long long pixels, int channels, void* dst, hipStream_t st);
int head_limb_launch(const ppn_conv_desc* d, const ppnconv::ConvSegment& s, hipStream_t st);  // conv_head.hip
int conv64_launch(const ppn_conv_desc* d, hipStream_t st);                                    // conv64.hip
int splitk_launch(const ppn_conv_desc* d, const ppnconv::ConvSegment& s, hipStream_t st);     // conv_splitk.hip
int stem3x3_launch(const ppn_conv_desc* d, hipStream_t st);                                   // stem3x3.hip
int block64_launch(const ppn_block_desc* d, hipStream_t st, const char** kname);              // block64.hip
int stem_launch(int dtype, int src_is_u8, const void* src, int batch, int h, int w, const float* weight,
                const float* scale, const float* shift, const float* mean, const float* stdv, void* out,
                hipStream_t st);                                                              // stem.hip
int stem01_launch(int dtype, int src_is_u8, const void* src, int batch, int h, int w, const float* w0,
                  const float* s0, const float* b0, const float* mean, const float* stdv, const float* w1,
                  const float* s1, const float* b1, void* out, hipStream_t st);               // stem01.hip
int stem012_launch(int dtype, int src_is_u8, const void* src, int batch, int h, int w, const float* w0, const float* s0,
                   const float* b0, const float* mean, const float* stdv, const float* w1, const float* s1,
                   const float* b1, const float* w2, const float* s2, const float* b2, const float* s3, const float* b3,
                   void* out_raw, void* out_act, hipStream_t st);                             // stem012.hip
int stem012_x3_launch(int src_is_u8, const void* src, int batch, int h, int w, const float* w0, const float* s0,
                      const float* b0, const float* mean, const float* stdv, const float* w1, const float* s1,
                      const float* b1, const float* w2, const float* s2, const float* b2, const float* s3, const float* b3,
                      void* out_raw, void* out_act, hipStream_t st);                          // stem012_x3.hip
bool stem_wgrad_supported(const ppn_wgrad_desc* d);                                           // stem_wgrad.hip
size_t stem_wgrad_workspace_bytes(const ppn_wgrad_desc* d);
int stem_wgrad_launch(const ppn_wgrad_desc* d, hipStream_t st);
}  // namespace ppn
