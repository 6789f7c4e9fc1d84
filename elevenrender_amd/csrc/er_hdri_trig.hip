// er_hdri_trig.hip -- fills the row and column tables of er_hdri_trig.h: one thread per column, then one per row, each calling the
// entry function that calls the bounce step's own device functions.  width + height threads; runs at er_render_begin and when an
// edit replaces the HDRI.
#include "er_hdri_trig.h"

using namespace erd;

__global__ __launch_bounds__(64) void er_hdri_trig_kernel(DevTex t, uint32_t* __restrict__ table) {
    const int w = t.width > 0 ? t.width : 0, h = t.height > 0 ? t.height : 0;
    const int i = (int)(blockIdx.x * 64u + threadIdx.x);
    if (i < w) {
        ((HdriCol*)table)[i] = hdri_col_entry(t, i);
    } else if (i - w < h) {
        ((HdriRow*)(table + hdri_trig_row_offset(t.width)))[i - w] = hdri_row_entry(t, i - w);
    }
}

void er_launch_hdri_trig(const DevTex& t, uint32_t* table, hipStream_t stream) {
    const long long n = (long long)(t.width > 0 ? t.width : 0) + (long long)(t.height > 0 ? t.height : 0);
    if (n == 0) return;
    hipLaunchKernelGGL(er_hdri_trig_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, t, table);
}

void er_hdri_trig_host(const DevTex& t, uint32_t* table) {
    HdriCol* cols = (HdriCol*)table;
    HdriRow* rows = (HdriRow*)(table + hdri_trig_row_offset(t.width));
    for (int x = 0; x < t.width; x++) cols[x] = hdri_col_entry(t, x);
    for (int y = 0; y < t.height; y++) rows[y] = hdri_row_entry(t, y);
}
