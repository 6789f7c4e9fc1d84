// er_hdri_trig.h -- row and column tables of the HDRI's next-event sample directions (DevScene::hdri_trig).
//
// The direction and the pdf of an HDRI texel drawn from the CDF (er_bounce.inc, src/kernel.cpp:549-553) go through four binary64
// polynomial transcendentals per opaque hit: er_cos(phi - PI), er_sin(phi - PI), er_cos(theta) of reverse_spherical_mapping and the
// er_sin(theta) of hdri_pdf.  phi is a function of the texel's column alone, theta of its row alone, so a width + height table holds
// every value these calls can produce for a CDF sample.  An entry is made by CALLING the functions of er_device.h -- inverse_transform_uv,
// rsm_column, rsm_row, hdri_pdf_sine, in the bounce step's own expression order -- so a table read is the bits the evaluation would
// give, and needs no argument about values.  One kernel fills it on the device (er_hdri_trig.hip) at er_render_begin and again when an
// edit replaces the HDRI; it lies behind the CDF's guide table in the same buffer.  ER_HDRI_TRIG_ON_DEVICE=1 (read by er_render_begin)
// leaves DevScene::hdri_trig null and the kernels evaluate: the A/B, and the other side of tests/test_gpu_hdri_trig.py.
#pragma once
#include "er_device.h"

namespace erd {

// 16 bytes per column x: what the step needs of texel column x of a CDF sample
struct HdriCol {
    float px, pz;      // er_cos(phi - PIF), -er_sin(phi - PIF) for phi = iu * 2 * PIF
    int32_t ix;        // f2i(iu * width): the column tex_uv / hdri_pdf index with
    float iu;          // inverse_transform_uv's u for nu = (float)x / (float)width
};
// 24 bytes per row y (the first 16 are the NEE sample's)
struct HdriRow {
    float py, a;       // -er_cos(theta), sqrtf(1 - py * py) for theta = iv * PIF
    int32_t iy;        // f2i(iv * height): the row tex_uv / hdri_pdf index with
    float sin_pdf;     // er_sin of hdri_pdf's own theta for row iy
    float iv;          // inverse_transform_uv's v for nv = (float)y / (float)height
    float sin_row;     // er_sin of hdri_pdf's own theta for row y itself (the MIS miss branch arrives with y, not through inverse_transform_uv)
};
static_assert(sizeof(HdriCol) == 16 && sizeof(HdriRow) == 24, "er_hdri_trig.h: table entry sizes");

#define ER_HT_HD __host__ __device__ __forceinline__

ER_HT_HD HdriCol hdri_col_entry(const DevTex& t, int x) {
    HdriCol c;
    float nu = (float)x / (float)t.width, iv;
    inverse_transform_uv(t, nu, 0.0f, c.iu, iv);
    rsm_column(c.iu, c.px, c.pz);
    c.ix = ermath::f2i(c.iu * t.width);
    return c;
}
ER_HT_HD HdriRow hdri_row_entry(const DevTex& t, int y) {
    HdriRow r;
    float nv = (float)y / (float)t.height, iu;
    inverse_transform_uv(t, 0.0f, nv, iu, r.iv);
    rsm_row(r.iv, r.py, r.a);
    r.iy = ermath::f2i(r.iv * t.height);
    r.sin_pdf = hdri_pdf_sine(t, r.iy);
    r.sin_row = hdri_pdf_sine(t, y);
    return r;
}

// words of the table for a width x height HDRI, and where its rows begin (words from the table's start)
ER_HT_HD size_t hdri_trig_row_offset(int width) { return (size_t)(width > 0 ? width : 0) * 4; }
ER_HT_HD size_t hdri_trig_words(int width, int height) { return hdri_trig_row_offset(width) + (size_t)(height > 0 ? height : 0) * 6; }

// the table of DevScene S (non-null), as the bounce step reads it; x in [0, width), y in [0, height)
__device__ __forceinline__ const HdriCol* hdri_trig_cols(const DevScene& S) { return (const HdriCol*)S.hdri_trig; }
__device__ __forceinline__ const HdriRow* hdri_trig_rows(const DevScene& S) { return (const HdriRow*)(S.hdri_trig + hdri_trig_row_offset(S.hdri_tex.width)); }

}  // namespace erd

// fills `table` (hdri_trig_words(t.width, t.height) words, 8-byte aligned) for HDRI descriptor `t` on `stream`
void er_launch_hdri_trig(const DevTex& t, uint32_t* table, hipStream_t stream);
// the same entries evaluated on the host (the kernel's twin: the functions are __host__ __device__, er_math.h is one implementation)
void er_hdri_trig_host(const DevTex& t, uint32_t* table);
