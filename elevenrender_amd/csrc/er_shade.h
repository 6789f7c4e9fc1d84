// er_shade.h + er_bounce.inc -- ONE iteration of the bounce loop of renderingKernel (reference src/kernel.cpp:508-593),
// shared by every schedule of this library (er_kernels.hip megakernel, er_wavefront.hip, er_stream.hip) and by the
// per-bounce debug trace (er_debug.hip).  The schedules differ only in WHEN they trace the rays this step asks for; the
// arithmetic -- and with it every bit of the image -- is written once: the statement sequence lives in er_bounce.inc,
// which each kernel #includes at the point where it shades (hooks below), this header holds what it calls.
//
// Why textual inclusion and not a function: the same statements behind an always-inlined function with reference
// parameters and a "sink" policy object cost the wavefront shade kernel 16 % and the fused kernel 12 % (measured on one
// box, round 2: 242 vs 209 ms of shade launches per 20 steps) -- identical static instruction mix, ~12 more spill
// stores + fills per 64-slot ticket ON THE HOT PATH, each a dependent memory round trip in a kernel that runs one wave
// per SIMD.  Included as text, the kernels compile to the round-1 code.
//
// The step is formulated so that it never waits for a shadow query: a query's outcome only selects which of two
// precomputed contributions is added to the path's radiance (c_vis / c_occ), so the caller traces the shadow ray
// whenever it likes and adds the selected contribution BEFORE it touches `light` again -- the order of the
// additions is that of the reference (emission + HDRI next-event estimate first, then the point-light sample).
//
// Three build-defined extensions live here, all off by default (= reference behaviour, bit for bit):
//
//   ER_FLAG_POINT_LIGHTS  (SURVEY.md 8 a15).  The reference never evaluates point lights: pointLight()
//       (src/kernel.cpp:269-301) has no caller, returns nothing on its lit path, and no command loads a light.
//       This build follows the author's sketch.  Per OPAQUE bounce, with count > 0 lights:
//         * ONE extra RNG draw, taken right after DisneySample's three (so a bounce draws, in order: opacity,
//           HDRI cdf, BRDF r1 r2 r3, light pick);
//         * light k = min(int(count * r), count - 1)      (:280; rnd.next() can return exactly 1.0);
//         * newDir = normalized(light.position - point), dist = |light.position - point|, point = Hit.position
//           (:282-284);
//         * shadow ray from point + newDir * 0.001 (:287); OCCLUDED iff some triangle is hit nearer than the light
//           (:289-291) -- both distances measured from the shadow ray's origin (the sketch measures both from
//           `point`, i.e. the same comparison shifted by the common 0.001 offset; measured from the origin the
//           test is "any hit with |Hit.position - origin| < |light - origin|", which the any-hit traversal can end
//           at the first certain occluder);
//         * pointLightValue = radiance / dist^2 (:295), contribution = value * DisneyEval(newDir) * |newDir.N| /
//           pdf with pdf = count / 2pi (:275, :299-300) -- the sketch's pdf, kept although a uniform pick has
//           probability 1/count: like the other reference quirks it defines the result;
//         * light += reduction * contribution, a separate addition after the HDRI term (reduction = the throughput
//           before this bounce's BRDF weight); an occluded light adds reduction * (0,0,0), as the sketch's early
//           `return Vector3()` would; a light whose DisneyEval is exactly zero (below the horizon) is skipped
//           altogether -- no shadow ray, no addition.
//       A point light is a delta light: BRDF sampling cannot hit it, so it takes MIS weight 1.
//
//   ER_FLAG_MIS.  The reference computes two weights hw, bw (src/kernel.cpp:571-572) and never applies them; the NEE
//       and the BRDF-sampled environment contribution are both counted in full.  Its hw/bw mix the pdfs of two
//       DIFFERENT directions (hdripdf of wihdri, brdfpdf of wibrdf), which is not a partition of unity, so they are
//       not applied as they stand.  With ER_FLAG_MIS this build applies the balance heuristic per direction:
//         * NEE sample wihdri:          weight 1 / (1 + DisneyPdf(wihdri) / p_hdri(wihdri));
//         * BRDF sample wibrdf that leaves the scene (the miss branch of the NEXT iteration, :517-522): weight
//           1 / (1 + p_hdri(texel the direction maps to) / p_brdf), p_brdf = the brdfpdf of the last opaque bounce
//           (camera rays and paths that never bounced opaquely: weight 1).
//         Written as 1 / (1 + ratio) so that the infinite p_hdri of HDRI row 0 (sin(theta) = 0, src/HDRI.cpp:101-107)
//         gives the limits 1 and 0 instead of inf / inf.
//       No extra RNG draws.
//
//   ER_FLAG_MESH_LIGHTS.  Next-event estimation of emissive triangles (mesh lights), combined with the BRDF-sampled hits on them by
//       the balance heuristic.  The kernels compile it in only where the template switch MESH is true (ER_BOUNCE_MESH below); the
//       instances without it are the code they were.
//         1. Emitters: a triangle whose material has emission_tex >= 0, or a constant emission of luminance > 0 (lum = 0.2126 R +
//            0.7152 G + 0.0722 B); weight w = area x lum, with the mean luminance of the texture's texels for textured emission.
//            Triangles of zero area or zero weight get no entry.  The table (er_lights.h, built on the device by er_lights.hip) lists
//            the emitters in ascending slot order with a normalised CDF; P(t) = w_t / W.
//         2. Draws: on every opaque bounce with a non-empty table, three more right after DisneySample's three -- r_pick, u1, u2 --
//            taken always, also when the sample is then skipped: an opaque bounce draws 7 times (HDRI cell, BRDF r1 r2 r3, r_pick,
//            u1, u2) after its opacity draw.
//         3. Sample: k = the first table entry with cdf > r_pick, clamped to count - 1; p = (1 - sqrt u1) v0 + sqrt u1 (1 - u2) v1 +
//            sqrt u1 u2 v2 on k's stored vertices; dir = normalized(p - hd.position), dist = |p - hd.position|; the shadow ray
//            leaves from hd.position + dir * 0.001 and is occluded iff a triangle other than k is hit nearer than |p - origin|
//            (ER_BOUNCE_LIGHT_QUERY with k's slot as the excluded one).
//         4. Le = the emission generate_hit_data would give at p's interpolated uv, times the opacity at p clamped to [0, 1] (the
//            probability that a hit there passes its opacity draw, the only case in which a hit adds its emission).
//         5. p_L = P(k) dist^2 / (A_k |cos_l|), cos_l = dot(k's geometric normal, dir): emitters are two-sided, as the emission a
//            hit adds is.
//         6. Contribution reduction * (Le * DisneyEval(wo, N, dir) * |dir . N| / p_L * w_nee), w_nee = 1 / (1 + DisneyPdf(wo, N,
//            dir) / p_L); skipped -- no ray, no addition -- when k is the triangle being shaded, when cos_l = 0, when DisneyEval
//            is exactly zero, or at the last bounce (bounce + 1 = max_bounces): the path ends there, so the BRDF-sampled ray that
//            would carry the other part of that light is never traced, and the sample would add w_nee of a path one segment longer
//            than the render without the flag counts (+0.8 % on the dim Cornell scene).  Added after the HDRI
//            term, as the point-light term is.
//         7. Emission found by a BRDF-sampled ray: the hd.emission term of c_vis / c_occ is multiplied by w_bsdf = 1 / (1 +
//            p_L(hit) / prev_pdf), p_L(hit) with the hit triangle's P, area and cos_l and the distance from the last opaque bounce
//            (path state `mesh_d`, the distance from that bounce to the current ray's origin, kept in ray_o.w of the wavefront and
//            streaming records).  Weight 1 for camera rays, for paths without an opaque bounce yet, for triangles not in the table,
//            and for a ray that has gone through a hit that failed its opacity draw since the last opaque bounce (mesh_d < 0 marks
//            it): the emitter sample's shadow ray treats every triangle as opaque, so it never makes a connection through a cut-out
//            and the BRDF-sampled ray carries that light alone.  (Until this was tested on a scene with cut-outs the weight was
//            applied there too, with the segments summed, and lost that light's w_nee share: DESIGN.md 3c.)  prev_pdf is carried
//            whenever the table is non-empty.
//         8. ER_FLAG_MIS (the HDRI weights) is independent of this flag.  A scene with an empty table renders exactly as without the
//            flag (the MESH = false instances run).  ER_FLAG_POINT_LIGHTS with this flag on a scene that has point lights and
//            emitters: er_render_begin returns ER_ERR_INVALID_ARG (both would need the one light-query record per slot).
//       Like the HDRI's next-event estimate, the shadow ray treats every triangle as opaque.
//   Parity for the extensions is UNPINNED by construction (the reference defines no result); the oracle mirrors all three
//   operation for operation (oracle/er_oracle.cpp) and the GPU tests require bit-equality with it.  For ER_FLAG_MESH_LIGHTS the oracle
//   takes the emitter order from the device (oracle_set_emitters), builds the table itself and answers the emitter shadow query by
//   brute force (tests/test_gpu_mesh_light_parity.py); tests/test_gpu_mesh_lights.py replays the table in numpy float32 bit for bit and
//   checks the schedules against each other and the estimator's mean against the render without the flag.
#pragma once
#include "er_device.h"
#include "er_hdri_trig.h"

namespace erd {

// host side: does this render need the MESH = true kernels (which are EXT = true as well)?  The bit is set in the scene descriptor only
// for a non-empty emitter table (er_render_begin).
static inline bool er_mesh_active(const DevScene& S) { return (S.ext_flags & ER_FLAG_MESH_LIGHTS) != 0; }
// host side: does this render need the EXT = true kernels?
static inline bool er_ext_active(const DevScene& S) {
    return (S.ext_flags & ER_FLAG_MIS) != 0 || ((S.ext_flags & ER_FLAG_POINT_LIGHTS) != 0 && S.light_count > 0) || er_mesh_active(S);
}

// ---- the emitter table of ER_FLAG_MESH_LIGHTS (layout: er_lights.h) ----
ERD const float* mesh_prob(const DevScene& S) { return S.mesh_lights; }
ERD const float* mesh_cdf(const DevScene& S) { return S.mesh_lights + S.tri_count; }
ERD uint32_t mesh_slot(const DevScene& S, uint32_t k) { return __builtin_bit_cast(uint32_t, S.mesh_lights[(size_t)S.tri_count + S.emitter_count + k]); }
// the first k with cdf[k] > r, clamped to n - 1 (r can be exactly 1.0, the last entry can round below it)
ERD uint32_t mesh_pick(const DevScene& S, float r) {
    const float* cdf = mesh_cdf(S);
    uint32_t lo = 0, hi = S.emitter_count;
    while (lo < hi) {
        const uint32_t m = lo + ((hi - lo) >> 1);
        if (cdf[m] > r) hi = m; else lo = m + 1;
    }
    return lo < S.emitter_count ? lo : S.emitter_count - 1;
}
// area and unit geometric normal of a slot's triangle: c = cross(v1 - v0, v2 - v0), A = 0.5 |c|, n = c / |c| (the builder's weights
// use the same expression for A)
ERD void mesh_tri(const DevScene& S, uint32_t slot, F3& v0, F3& v1, F3& v2, F3& ng, float& area) {
    float4 a, b, c;
    load_verts(S, slot, v0, v1, v2, a, b, c);
    const F3 cr = cross(v1 - v0, v2 - v0);
    const float len = length(cr);
    area = 0.5f * len;
    ng = cr / len;
}

// End of a path, src/kernel.cpp:597-645: clamp to [0,10], NaN gate, running mean over `sa` (which starts at 1, so after
// n samples the planes hold sum/(n+1)); the DENOISE plane is never written.  Returns the new sample count.
ERD uint32_t accumulate_sample(const DevScene& S, uint32_t idx, uint32_t sa, F3 light, F3 aov_n, F3 aov_t, F3 aov_b) {
    const size_t npx = (size_t)S.x_res * S.y_res;
    light = f3(clampf(light.x, 0, 10), clampf(light.y, 0, 10), clampf(light.z, 0, 10));
    if (!(light.x != light.x) && !(light.y != light.y) && !(light.z != light.z)) {
        const float k = ((float)sa) / ((float)(sa + 1));
        const float inv = (float)(sa + 1);
        const F3 vals[4] = {light, aov_n, aov_t, aov_b};
        const int planes[4] = {ER_PASS_BEAUTY, ER_PASS_NORMAL, ER_PASS_TANGENT, ER_PASS_BITANGENT};
#pragma unroll
        for (int q = 0; q < 4; q++) {
            float4* pp = S.passes + er_pass_index(npx, planes[q], idx);      // (the four are neighbours: one 64-byte run)
            float4 p = *pp;
            if (sa > 0) { p.x *= k; p.y *= k; p.z *= k; }
            p.x += vals[q].x / inv; p.y += vals[q].y / inv; p.z += vals[q].z / inv;
            *pp = p;
        }
        sa++;
    }
    return sa;
}

}  // namespace erd
