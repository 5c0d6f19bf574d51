// bb_rgbd.h -- onboard RGB-D cameras (bb_rgbd.hip), shared with the C-ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bb_model.h"
#include "bb_render.h"

namespace bb {

// scratch the launch needs: per (env, camera) scene
size_t rgbd_scene_bytes(int n);
// rgbd float[n][2][4][H][W] (planes R, G, B, D), ids int8[n][2][H][W] (may be NULL), rel_ts float[n] (may be NULL)
int launch_rgbd(bool fp64, const ModelT<float>& m, const CamRig& rig, const RenderDev& d, int H, int W, int every,
                int force, double dt, void* scenes, float* rgbd, float* rel_ts, int8_t* ids, hipStream_t s);

}  // namespace bb
