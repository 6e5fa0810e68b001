// render.h -- entry point of the host driver (render.cpp).
#pragma once
#include "scene.h"
namespace rdr {
void render(const Scene &scene, const rdr_render_options &opt, float *image, const float *d_image,
            const rdr_dscene_desc *d_scene, float *screen_gradient_image, float *debug_image);
// rdr_debug_grad_scatter (include/redner_amd.h): lives in render.cpp because the replica layout that rdr::accum reads is a
// device symbol of the translation unit that instantiates the stage kernels (hip/exec.h: g_rep)
void debug_grad_scatter(const Scene &scene, const rdr_dscene_desc &d_scene, size_t job_samples, int op, bool plain, int num_lanes,
                        const uint8_t *active, const int32_t *target, const int32_t *index, const double *values);
// rdr_debug_lane_park: beside the stages whose parks it stands for; returns the number of columns (stages_fwd.h: kMaxParkDoubles)
int debug_lane_park(int num_lanes, const uint8_t *active, const double *in, double *out);
}
