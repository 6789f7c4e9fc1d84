// er_bounce.inc -- the statements of ONE bounce-loop iteration (reference src/kernel.cpp:508-593), #included by every
// kernel that shades (see er_shade.h for the rules of the two extensions and for why this is text, not a function).
//
// In scope at the point of inclusion (all plain locals of the including kernel):
//   COUNT, EXT          compile-time bools (EXT = false compiles the extensions out)
//   ER_BOUNCE_FUSE      macro, optional (default true): a compile-time bool; false compiles the fused-texel fetch of generate_hit_data out
//   ER_BOUNCE_MESH      macro, optional (default false): a compile-time bool; true compiles ER_FLAG_MESH_LIGHTS in (needs EXT)
//   ER_BOUNCE_SKIP_EQUAL macro, optional (default true): a compile-time bool; false hands every shadow query to the hooks even when its
//                       two outcomes are the same addend (the debug pixel trace: its records are compared with the oracle's, which always traces)
//   ER_BOUNCE_KEEP_LAST macro, optional (default false): a compile-time bool; true computes the continuation -- the BRDF-sampled direction, its
//                       pdf and BRDF term, `reduction`, `prev_pdf`, the new `ray` -- on the path's last iteration as well, where nothing
//                       reads it after `done` (the debug pixel trace: its records carry the next direction and the throughput)
//   S                   the DevScene
//   Ray      ray        in: the ray that was traced; out: the continuation ray (unchanged when it left the scene)
//   int      hslot      its closest hit (triangle slot), or < 0
//   uint32_t rs         the pixel's RNG state
//   F3       light, reduction;  uint32_t bounce      the path state of src/kernel.cpp:496-506
//   float    prev_pdf   ER_FLAG_MIS / ER_FLAG_MESH_LIGHTS: brdfpdf of the last opaque bounce, < 0 before the first one (read only if EXT)
//   float    mesh_d     ER_FLAG_MESH_LIGHTS: distance from the last opaque bounce to ray.o, < 0 once the ray has gone through a hit that failed its
//                       opacity draw (read and written only if ER_BOUNCE_MESH)
//   bool     done       set when the path ends with this step (left the scene, or the bounce limit is reached)
//   bool     pending, lpending   set when an HDRI / a point-light shadow query was handed to the hooks
//   unsigned c_shaded, c_texels, c_hdri   counters
//   ER_TP(n)            section stamp of a diagnostic build (tools/shader_sections.py); nothing in the product
// Hooks (macros defined by the including kernel; expanded where the values are produced, so nothing stays live longer):
//   ER_BOUNCE_HDRI_QUERY(sr, self_slot, d_self, c_vis, c_occ)
//       HDRI shadow ray `sr`; occluded iff its closest hit is a triangle other than self_slot, i.e. iff some other
//       triangle is hit nearer than d_self (the distance at which sr re-hits the triangle it leaves; inf if it does
//       not).  Then light += occluded ? c_occ : c_vis.
//   ER_BOUNCE_LIGHT_QUERY(lr, self_slot, limit, l_vis, l_occ)
//       point-light (self_slot -1) or emitter (self_slot = the emitter's slot) shadow ray; occluded iff some triangle other than
//       self_slot is hit nearer than `limit`.  Then, AFTER the HDRI term, light += occluded ? l_occ : l_vis.
//   ER_BOUNCE_FIRST_HIT(n, t, b)       first-bounce AOVs (src/kernel.cpp:581-585)
// A kernel may trace at once inside a hook and add to `light` itself (megakernel, debug trace), or record the query and
// add the selected contribution before `light` is touched again (wavefront, fused).
#ifndef ER_BOUNCE_FUSE
#define ER_BOUNCE_FUSE true
#endif
#ifndef ER_BOUNCE_SKIP_EQUAL
#define ER_BOUNCE_SKIP_EQUAL true
#endif
#ifndef ER_BOUNCE_KEEP_LAST
#define ER_BOUNCE_KEEP_LAST false
#endif
{
    // A shadow query only selects one of two addends that are both known before it is traced.  Where the two are the same bits the verdict
    // cannot change `light`, and the query is not issued: the addend is added at once.  The common case is a dead path -- `reduction` exactly
    // (0, 0, 0) after a bounce whose DisneyEval was zero (a back-facing hit) -- which still has to trace its closest-hit rays (their hits
    // decide how many numbers the sample draws) but none of its shadow rays.  DevScene::trace_every_query (a scalar load) switches the rule off.
    const bool er_skip_equal = (ER_BOUNCE_SKIP_EQUAL) && S.trace_every_query == 0u;
    const int hw = S.hdri_tex.width, hh = S.hdri_tex.height;
    const bool er_mis = EXT && (S.ext_flags & ER_FLAG_MIS) != 0;
#ifdef ER_BOUNCE_MESH
    constexpr bool er_mesh = EXT && (ER_BOUNCE_MESH);      // (a non-empty emitter table: the host runs these instances only then)
#else
    constexpr bool er_mesh = false;
#endif
    if (hslot < 0) {
        // src/kernel.cpp:517-522
        float u, v;
        spherical_mapping(-1 * ray.d, u, v);
        if (EXT) {
            F3 er_env = tex_filtered(S, S.hdri_tex, u, v);
            if (er_mis && prev_pdf >= 0.0f) {   // balance heuristic for the BRDF-sampled direction that left the scene
                // (hdri_pdf; the sine of its row from the row table where there is one and the row lies inside the image)
                const int er_mx = ermath::f2i(u * hw), er_my = ermath::f2i(v * hh);
                const float er_ms = (S.hdri_trig != nullptr && (unsigned)er_my < (unsigned)hh) ? hdri_trig_rows(S)[er_my].sin_row : hdri_pdf_sine(S.hdri_tex, er_my);
                const float er_ph = hdri_pdf_of(S, tex_coords(S, S.hdri_tex, er_mx, er_my), er_ms);
                er_env = er_env * (1.0f / (1.0f + er_ph / prev_pdf));
                if (COUNT) c_texels++;
            }
            light = light + reduction * er_env;
        } else {
            light = light + reduction * tex_filtered(S, S.hdri_tex, u, v);
        }
        if (COUNT) c_texels++;
        done = true;
    } else {
        c_shaded++;
        ER_TP(2);
        HitFull hit;
        full_hit(S, (uint32_t)hslot, ray, hit);
        const ErMaterial& mat = S.materials[hit.material];
        HitData hd;
        generate_hit_data<COUNT, ER_BOUNCE_FUSE>(S, mat, hit, hd, c_texels);
        int shader = mat.albedo_shader_id;
        if (shader != -1) {   // asl_shade placeholder, src/shader.cpp:6-10, src/shader.h:10-11
            hd.albedo = f3s(0);
            if (shader >= 0 && shader < 4) hd.albedo = f3(1, 1, 0);
        }
        if (rng_next(rs) <= hd.opacity) {
            F3 wo = ray.d * -1.0f;
            F3 N = hd.normal;
            c_hdri++;
            ER_TP(3);
            int count = er_cdf_search(S.hdri_cdf, hw * hh, S.hdri_guide, S.hdri_buckets, rng_next(rs));   // == HDRI::binarySearch
            // (for a power-of-two width and a non-negative index the division is a shift and a mask -- the same integers)
            const bool hw_pow2 = (hw & (hw - 1)) == 0 && hw > 0 && count >= 0;
            const int er_cx = hw_pow2 ? (int)((unsigned)count & (unsigned)(hw - 1)) : count % hw;
            const int er_cy = hw_pow2 ? (int)((unsigned)count >> (31 - __builtin_clz((unsigned)hw))) : count / hw;
            float tcx = (float)er_cx, tcy = (float)er_cy;
            float d1 = rng_next(rs), d2 = rng_next(rs), d3 = rng_next(rs);
            const bool er_lights = EXT && !er_mesh && (S.ext_flags & ER_FLAG_POINT_LIGHTS) != 0 && S.light_count > 0;
            float er_rl = 0.0f;
            if (er_lights) er_rl = rng_next(rs);     // the light pick: one extra draw, right after DisneySample's three
            float er_mp = 0.0f, er_mu1 = 0.0f, er_mu2 = 0.0f;
            if (er_mesh) { er_mp = rng_next(rs); er_mu1 = rng_next(rs); er_mu2 = rng_next(rs); }   // emitter pick and point: always three
            ER_TP(4);
            // The path's last iteration: the three BRDF draws above are taken, but the continuation they feed -- the sampled direction, its pdf
            // and BRDF term, `reduction`, `prev_pdf`, the new ray -- goes to variables that nothing reads after `done`, and is not computed.
            const bool er_last = !(ER_BOUNCE_KEEP_LAST) && bounce + 1u >= S.max_bounces;
            F3 wibrdf = f3s(0);
            if (!er_last) wibrdf = DisneySample(hd, wo, N, d1, d2, d3);
            // The sampled texel's direction and pdf (inverse_transform_uv, reverse_spherical_mapping, tex_uv, hdri_pdf): the transcendentals
            // depend on the texel's column and row alone and come from the tables of er_hdri_trig.h where there are some -- the bits the
            // functions below gave when the table was filled with them.  (A search that found nothing, count = -1, is not a texel: evaluated.)
            float er_px, er_pz, er_py, er_a, er_sin;
            int er_ix, er_iy;
            if (S.hdri_trig != nullptr && (unsigned)count < (unsigned)(hw * hh)) {
                const HdriCol er_c = hdri_trig_cols(S)[er_cx];
                const HdriRow er_r = hdri_trig_rows(S)[er_cy];
                er_px = er_c.px; er_pz = er_c.pz; er_ix = er_c.ix;
                er_py = er_r.py; er_a = er_r.a; er_iy = er_r.iy; er_sin = er_r.sin_pdf;
            } else {
                float nu = tcx / (float)hw, nv = tcy / (float)hh;
                float iu, iv;
                inverse_transform_uv(S.hdri_tex, nu, nv, iu, iv);
                rsm_column(iu, er_px, er_pz);
                rsm_row(iv, er_py, er_a);
                er_ix = ermath::f2i(iu * hw); er_iy = ermath::f2i(iv * hh);      // (tex_uv's and hdri_pdf's texel: the same one)
                er_sin = hdri_pdf_sine(S.hdri_tex, er_iy);
            }
            F3 wihdri = normalized(f3(er_a * er_px, er_py, er_a * er_pz)) * -1.0f;      // reverse_spherical_mapping's result
            F3 hdriValue = tex_coords(S, S.hdri_tex, er_ix, er_iy);                     // tex_uv; hdri_pdf reads this texel too: fetched once
            if (COUNT) c_texels += 2;
            F3 evalh = DisneyEval(hd, wo, N, wihdri);
            float hdripdf = hdri_pdf_of(S, hdriValue, er_sin);
            float absdot = __builtin_fabsf(dot(wihdri, N));
            // The reference always traces the shadow ray (src/kernel.cpp:555-562); a hit on another triangle zeroes
            // hdriValue.  Both outcomes are computed here with the reference's expression; when the BRDF term is
            // exactly zero, or the two addends are the same bits for another reason, they coincide and the query is skipped.
            float er_wnee = 1.0f;
            if (er_mis) er_wnee = 1.0f / (1.0f + DisneyPdf(hd, wo, N, wihdri) / hdripdf);   // balance heuristic, NEE direction
            F3 er_em = hd.emission;
            if (er_mesh && prev_pdf >= 0.0f && mesh_d >= 0.0f) {
                // emission found by a BRDF-sampled ray: balance heuristic against the emitter sample (rule 7); weight 1 after an opacity
                // pass-through, a connection the emitter sample never makes (its shadow ray treats every triangle as opaque)
                const float er_ph = mesh_prob(S)[hslot];
                if (er_ph > 0.0f) {
                    F3 er_a, er_b, er_c, er_ng;
                    float er_area;
                    mesh_tri(S, (uint32_t)hslot, er_a, er_b, er_c, er_ng, er_area);
                    const float er_dh = mesh_d + length(hit.position - ray.o);
                    const float er_pl = er_ph * (er_dh * er_dh) / (er_area * __builtin_fabsf(dot(er_ng, ray.d)));
                    er_em = er_em * (1.0f / (1.0f + er_pl / prev_pdf));
                }
            }
            F3 c_vis = er_mis ? reduction * (er_em + (hdriValue * evalh * absdot / hdripdf) * er_wnee)
                              : reduction * (er_em + hdriValue * evalh * absdot / hdripdf);
            const F3 c_occ = er_mis ? reduction * (er_em + (f3s(0) * evalh * absdot / hdripdf) * er_wnee)
                                    : reduction * (er_em + f3s(0) * evalh * absdot / hdripdf);
            if ((evalh.x != 0.0f || evalh.y != 0.0f || evalh.z != 0.0f) && !(er_skip_equal && same_bits(c_vis, c_occ))) {
                // shadow query needed: occluded iff the closest hit is another triangle
                Ray sr = make_ray(hd.position + N * 0.001f, wihdri);
                F3 v0, v1, v2;
                float4 qa, qb, qc4;
                load_verts(S, (uint32_t)hslot, v0, v1, v2, qa, qb, qc4);
                float su, sv, st, d_self = __builtin_inff();
                if (tri_mt(v0, v1, v2, sr, su, sv, st)) d_self = candidate_distance(S, (uint32_t)hslot, v0, v1, v2, sr, su, sv, st);
                ER_BOUNCE_HDRI_QUERY(sr, hslot, d_self, c_vis, c_occ);
                pending = true;
            } else {
                light = light + c_vis;
            }
            if (er_lights) {
                // the author's sketch pointLight(), src/kernel.cpp:269-301 (rules: er_shade.h)
                int er_k = ermath::f2i((float)S.light_count * er_rl);                    // :280
                er_k = er_k > (int)S.light_count - 1 ? (int)S.light_count - 1 : er_k;   // rnd.next() can return exactly 1.0
                const ErPointLight er_L = S.lights[er_k];
                const F3 er_lpos = f3(er_L.position.x, er_L.position.y, er_L.position.z);
                const F3 er_toL = er_lpos - hd.position;
                const F3 er_dir = normalized(er_toL);                                    // :282
                const float er_dist = length(er_toL);                                    // :284
                const Ray er_lr = make_ray(hd.position + er_dir * 0.001f, er_dir);       // :287
                const float er_limit = length(er_lpos - er_lr.o);
                const F3 er_value = f3(er_L.radiance.x, er_L.radiance.y, er_L.radiance.z) / (er_dist * er_dist);   // :295
                const F3 er_evall = DisneyEval(hd, wo, N, er_dir);                       // :297
                const float er_lpdf = ((float)S.light_count) / (2.0f * PIF);             // :275
                // a light whose BRDF term is exactly zero (below the shading normal's horizon) is skipped: no ray, no addition
                if (er_evall.x != 0.0f || er_evall.y != 0.0f || er_evall.z != 0.0f) {
                    const F3 er_pl = er_value * er_evall * __builtin_fabsf(dot(er_dir, N)) / er_lpdf;   // :299-300
                    const F3 er_lv = reduction * er_pl, er_lo = reduction * f3s(0);
                    // (the same addend either way: added now, which is its place -- after the HDRI term -- only if that term is in `light` already)
                    if (er_skip_equal && !pending && same_bits(er_lv, er_lo)) {
                        light = light + er_lv;
                    } else {
                        ER_BOUNCE_LIGHT_QUERY(er_lr, -1, er_limit, er_lv, er_lo);
                        lpending = true;
                    }
                }
            }
            if (er_mesh && bounce + 1u < S.max_bounces) {
                // an emitter sample (rules 3-6, er_shade.h); none at the last bounce, whose BRDF-sampled partner is never traced
                const uint32_t er_k = mesh_slot(S, mesh_pick(S, er_mp));
                if ((int)er_k != hslot) {
                    F3 er_a, er_b, er_c, er_ng;
                    float er_area;
                    mesh_tri(S, er_k, er_a, er_b, er_c, er_ng, er_area);
                    const float er_su = __builtin_sqrtf(er_mu1);
                    const float er_b1 = er_su * (1.0f - er_mu2), er_b2 = er_su * er_mu2;
                    const F3 er_p = er_a * (1.0f - er_su) + er_b * er_b1 + er_c * er_b2;
                    const F3 er_toL = er_p - hd.position;
                    const F3 er_dir = normalized(er_toL);
                    const float er_dist = length(er_toL);
                    const float er_cosl = dot(er_ng, er_dir);
                    const F3 er_evall = er_cosl != 0.0f ? DisneyEval(hd, wo, N, er_dir) : f3s(0);
                    if (er_evall.x != 0.0f || er_evall.y != 0.0f || er_evall.z != 0.0f) {
                        // Le: the emission generate_hit_data would give at p's uv, times the opacity there (rule 4)
                        const float4* er_q = S.tri_attr + (size_t)er_k * ER_ATTR_PIECES;
                        const float4 er_q4 = er_q[4], er_q5 = er_q[5];
                        const ErMaterial& er_m = S.materials[__builtin_bit_cast(int, er_q[6].x)];
                        const float er_tu = er_q4.z + (er_q5.x - er_q4.z) * er_b1 + (er_q5.z - er_q4.z) * er_b2;
                        const float er_tv = er_q4.w + (er_q5.y - er_q4.w) * er_b1 + (er_q5.w - er_q4.w) * er_b2;
                        F3 er_le = er_m.emission_tex < 0 ? f3(er_m.emission.x, er_m.emission.y, er_m.emission.z)
                                                         : tex_filtered(S, S.textures[er_m.emission_tex], er_tu, er_tv);
                        const float er_op = er_m.opacity_tex < 0 ? er_m.opacity : tex_filtered(S, S.textures[er_m.opacity_tex], er_tu, er_tv).x;
                        er_le = er_le * clampf(er_op, 0.0f, 1.0f);
                        if (COUNT) c_texels += (er_m.emission_tex < 0 ? 0 : 1) + (er_m.opacity_tex < 0 ? 0 : 1);
                        const float er_lpdf = mesh_prob(S)[er_k] * (er_dist * er_dist) / (er_area * __builtin_fabsf(er_cosl));
                        const float er_wl = 1.0f / (1.0f + DisneyPdf(hd, wo, N, er_dir) / er_lpdf);
                        const F3 er_ml = er_le * er_evall * __builtin_fabsf(dot(er_dir, N)) / er_lpdf * er_wl;
                        const F3 er_lv = reduction * er_ml, er_lo = reduction * f3s(0);
                        if (er_skip_equal && !pending && same_bits(er_lv, er_lo)) {      // (as for a point light)
                            light = light + er_lv;
                        } else {
                            const Ray er_lr = make_ray(hd.position + er_dir * 0.001f, er_dir);
                            ER_BOUNCE_LIGHT_QUERY(er_lr, (int)er_k, length(er_p - er_lr.o), er_lv, er_lo);
                            lpending = true;
                        }
                    }
                }
            }
            ER_TP(5);
            if (!er_last) {
                float brdfpdf = DisneyPdf(hd, wo, N, wibrdf);
                reduction = reduction * (DisneyEval(hd, wo, N, wibrdf) * __builtin_fabsf(dot(wibrdf, N)) / brdfpdf);
                if (er_mis || er_mesh) prev_pdf = brdfpdf;
                ray = make_ray(hit.position + wibrdf * 0.001f, wibrdf);
            }
            if (bounce == 0) { ER_BOUNCE_FIRST_HIT(hd.normal, hd.tangent, hd.bitangent); }
            if (er_mesh) mesh_d = 0.001f;          // (the new ray leaves 0.001 away from the bounce)
        } else {
            if (er_mesh) mesh_d = -1.0f;           // an opacity pass-through: no emitter sample reaches what this ray finds (rule 7)
            ray = make_ray(hit.position + ray.d * 0.001f, ray.d);
        }
        ER_TP(6);
        bounce++;
        if (bounce >= S.max_bounces) done = true;
    }
}
