// bb_encoder_rgbd.h -- the fused frozen RGB-D encoder (bb_encoder_rgbd.hip), shared with the C-ABI.
// It takes bb_encoder.h's EncArgs: w1 is [32][4][3][3], an image is four contiguous 64x64 planes
// (R, G, B, D) at images + i * image_stride, and ws.part1 holds conv1's channel sums per workgroup.
#pragma once
#include "bb_encoder.h"

namespace bb {

long long rgbd_encoder_workspace_bytes(long long n);
int launch_rgbd_encoder(EncArgs a, float* ws, hipStream_t s);

}  // namespace bb
