// bb_view.h -- world-view RGB renderer (bb_view.hip), shared with the C-ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bb_model.h"
#include "bb_render.h"

namespace bb {

// MuJoCo's free camera, resolved on the host in double
struct ViewCam {
  float R[9];        // camera->world rotation, row-major (columns: right, up, -forward)
  double rel[3];     // camera origin - base body origin = lookat_offset - distance * forward
  float tan_half;    // tan(fovy / 2)
};

// scratch the launch needs: one scene per view
size_t view_scene_bytes(int n_views);
// rgb uint8[n_views][H][W][3], ids int8[n_views][H][W] (may be NULL); env_ids int32[n_views] on the device
int launch_view(bool fp64, const ModelT<float>& m, const RenderDev& d, const ViewCam& cam, const int32_t* env_ids,
                int n_views, int H, int W, void* scenes, uint8_t* rgb, int8_t* ids, hipStream_t s);

}  // namespace bb
