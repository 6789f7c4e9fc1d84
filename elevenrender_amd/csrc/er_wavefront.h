// er_wavefront.h -- per-slot path state and queues of the wavefront schedule (er_wavefront.hip).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/eleven_hip.h"

struct DevScene;

#define ER_WF_FINALIZE_ONLY 0x80000000u   // queue entry flag: no ray this iteration, only finalise the path

// reduc.w of a slot: bounce (bits 0-15) | HDRI shadow query pending (bit 16) | light query pending (bit 17)
#define ER_SLOT_BOUNCE_MASK 0xFFFFu
#define ER_SLOT_PENDING 0x10000u
#define ER_SLOT_LPENDING 0x20000u
static_assert(ER_MAX_BOUNCES <= ER_SLOT_BOUNCE_MASK && ER_SLOT_PENDING == ER_SLOT_BOUNCE_MASK + 1u && ER_SLOT_LPENDING == 2u * ER_SLOT_PENDING,
              "a bounce count of up to ER_MAX_BOUNCES (er_render_begin refuses more) must fit below the flag bits of reduc.w");

// indices into WfState::counts.  Every counter sits on its own 128-byte line: they are hammered by
// device-scope atomics from every wave, and words that share a line serialise on one L2 channel.
#define WF_LINE 32
#define WF_NC 0                   // [2] closest-queue lengths, by parity (WF_NC, WF_NC + WF_LINE)
#define WF_NS (2 * WF_LINE)       // [2] shadow-queue lengths, by parity
#define WF_TS (4 * WF_LINE)       // shade ticket
#define WF_TT (5 * WF_LINE)       // [8] trace tickets, one per XCD range (WF_TT + x * WF_LINE)
#define WF_COUNTS (13 * WF_LINE)
#define WF_PAR(p) ((p) * WF_LINE)

// One slot per owned pixel lane (owned_tile_count * 64).  All records are 16 bytes so a lane moves
// its state with dwordx4 accesses.
struct WfState {
    float4* ray_o;     // closest-hit ray origin (xyz), w = distance from the last opaque bounce (ER_FLAG_MESH_LIGHTS; 0 otherwise)
    float4* ray_d;     // closest-hit ray direction (xyz), w = brdfpdf of the last opaque bounce (ER_FLAG_MIS; < 0 none)
    int* hit;          // triangle slot of the closest hit, -1 = miss (written by trace)
    int* hit2;         // second surviving candidate (exact metric decides in shade), -1 none, -2 = re-trace exactly
    float4* light;     // xyz = accumulated radiance of the current path, w = bits(RNG state)
    float4* reduc;     // xyz = path throughput, w = bits(bounce | pending-shadow flag)
    uint32_t* left;    // samples still to finish for this pixel in this call (incl. the current one)
    float4* aov_n;     // first-bounce normal / tangent / bitangent (src/kernel.cpp:581-585)
    float4* aov_t;
    float4* aov_b;
    float4* sh_o;      // shadow ray origin (xyz), w = bits(triangle slot the ray leaves)
    float4* sh_d;      // shadow ray direction (xyz), w = distance at which the ray re-hits that triangle (inf if not)
    float4* c_vis;     // contribution to add if the shadow ray is unoccluded
    float4* c_occ;     // ... if it is occluded
    int* occluded;     // written by trace: 0 no, 1 yes, 2 = decide among occ_a/occ_b by exact metric, 3 = re-trace exactly
    int* occ_a;
    int* occ_b;
    uint32_t* q[2];    // closest queues (slot | flags), ping-pong by iteration parity
    uint32_t* qs[2];   // shadow queues (slot)
    uint32_t* counts;  // WF_COUNTS words
    uint2* spill;      // per persistent trace wave: ER_STACK8 x 64 stack entries beyond the LDS levels (er_trav.h)
    int* shade_stack;  // per shade wave: ER_BVH_MAX_DEPTH x 64 ints, the stack of the rare exact re-trace (in LDS until round 5: 16 KB per wave at depth 64)
    uint32_t slots;    // owned_tile_count * 64.  With ER_FLAG_POINT_LIGHTS or ER_FLAG_MESH_LIGHTS the shadow records (sh_o, sh_d, c_vis, c_occ,
                       // occluded, occ_a, occ_b) have 2 * slots entries: [slot] = the HDRI query, [slot + slots] = the
                       // light query of the same bounce; shadow-queue entries are these indices
    uint32_t pool, pools;   // this state drives the owned tiles t with t % pools == pool (see er_api.cpp: slot pools)
};

// ---- the slot protocol between the tracers and the shading step, stated once for this schedule and the streaming one ----
// (er_stream.hip keeps the same fields slot by slot in StState).  The including kernel file names field f of record i with
// ER_SLOT(f, i); everything else about the two layouts stays its own.  Text, for the reason er_shade.h gives: the statements work
// on the shading step's locals (S, stack, light, reduction, rs, ray, bounce, prev_pdf, mesh_d, pending, lpending, the counters).
// The hooks of er_bounce.inc that write the query and first-hit records are er_slot_bounce.inc.

// what the finished traversal T leaves in its ray's record q (the codes: er_trav.h); `certain`: a step found a certain occluder
#define ER_SLOT_WRITE_RESULT(q, T, certain)                                                            \
    {                                                                                                  \
        if ((T).shadow) {                                                                              \
            ER_SLOT(occluded, q) = trav_shadow_code(T, certain);                                       \
            ER_SLOT(occ_a, q) = (T).s0;                                                                \
            ER_SLOT(occ_b, q) = (T).s1;                                                                \
        } else {                                                                                       \
            ER_SLOT(hit, q) = trav_hit(T);                                                             \
            ER_SLOT(hit2, q) = trav_hit2(T);                                                           \
        }                                                                                              \
    }
// a fresh sample: camera ray `ray` of a pixel whose RNG state is `rs` after the ray's draws
#define ER_SLOT_RESET(i, ray, rs)                                                                     \
    ER_SLOT(ray_o, i) = make_float4((ray).o.x, (ray).o.y, (ray).o.z, 0.0f);                            \
    ER_SLOT(ray_d, i) = make_float4((ray).d.x, (ray).d.y, (ray).d.z, -1.0f);                           \
    ER_SLOT(light, i) = make_float4(0.0f, 0.0f, 0.0f, __builtin_bit_cast(float, (rs)));               \
    ER_SLOT(reduc, i) = make_float4(1.0f, 1.0f, 1.0f, __builtin_bit_cast(float, 0u));                 \
    ER_SLOT(aov_n, i) = make_float4(0, 0, 0, 0);                                                       \
    ER_SLOT(aov_t, i) = make_float4(0, 0, 0, 0);                                                       \
    ER_SLOT(aov_b, i) = make_float4(0, 0, 0, 0)
// the path state of slot i: declares light, reduction, packed and bounce, sets rs
#define ER_SLOT_LOAD(i)                                                                                \
    const float4 L4 = ER_SLOT(light, i), R4 = ER_SLOT(reduc, i);                                       \
    F3 light = f3(L4.x, L4.y, L4.z), reduction = f3(R4.x, R4.y, R4.z);                                 \
    rs = __builtin_bit_cast(uint32_t, L4.w);                                                           \
    const uint32_t packed = __builtin_bit_cast(uint32_t, R4.w);                                        \
    uint32_t bounce = packed & ER_SLOT_BOUNCE_MASK
// the ray that was traced for slot i, with what rides in its w components
#define ER_SLOT_LOAD_RAY(i)                                                                            \
    {                                                                                                  \
        const float4 o = ER_SLOT(ray_o, i), d = ER_SLOT(ray_d, i);                                     \
        ray.o = f3(o.x, o.y, o.z);                                                                     \
        ray.d = f3(d.x, d.y, d.z);                                                                     \
        if (MESH) mesh_d = o.w;                                                                        \
        if (EXT) prev_pdf = d.w;                                                                       \
    }
// ... and back (light alone: a path that is over keeps only its radiance and the RNG state)
#define ER_SLOT_STORE_LIGHT(i) ER_SLOT(light, i) = make_float4(light.x, light.y, light.z, __builtin_bit_cast(float, rs))
#define ER_SLOT_STORE(i, with_ray)                                                                     \
    if (with_ray) {                                                                                    \
        ER_SLOT(ray_o, i) = make_float4(ray.o.x, ray.o.y, ray.o.z, MESH ? mesh_d : 0.0f);              \
        ER_SLOT(ray_d, i) = make_float4(ray.d.x, ray.d.y, ray.d.z, EXT ? prev_pdf : -1.0f);            \
    }                                                                                                  \
    ER_SLOT_STORE_LIGHT(i);                                                                            \
    ER_SLOT(reduc, i) = make_float4(reduction.x, reduction.y, reduction.z,                            \
                                    __builtin_bit_cast(float, bounce | (pending ? ER_SLOT_PENDING : 0u) | ((EXT && lpending) ? ER_SLOT_LPENDING : 0u)))
// the pending query of shadow record q adds its addend to `light`: `code` is the query's verdict (er_trav.h trav_shadow_code);
// ER_SLOT_ADD_QUERY takes a certain one (0 / 1), ER_SLOT_RESOLVE_QUERY settles an ambiguous one first
#define ER_SLOT_ADD_QUERY(q, code)                                                                     \
    {                                                                                                  \
        const uint32_t aq = (q);                                                                       \
        const float4 c = (code) ? ER_SLOT(c_occ, aq) : ER_SLOT(c_vis, aq);                             \
        light = light + f3(c.x, c.y, c.z);                                                             \
    }
#define ER_SLOT_RESOLVE_QUERY(q, code)                                                                 \
    {                                                                                                  \
        const uint32_t rq = (q);                                                                       \
        int occ = (code);                                                                              \
        if (occ >= 2) {                                                                                \
            float4 so = ER_SLOT(sh_o, rq), sd = ER_SLOT(sh_d, rq);                                     \
            Ray sr;                                                                                    \
            sr.o = f3(so.x, so.y, so.z);                                                               \
            sr.d = f3(sd.x, sd.y, sd.z);                                                               \
            occ = resolve_shadow<COUNT>(S, stack, sr, __builtin_bit_cast(int, so.w), sd.w, occ, ER_SLOT(occ_a, rq), ER_SLOT(occ_b, rq), c_nodes, c_tris) ? 1 : 0; \
        }                                                                                              \
        ER_SLOT_ADD_QUERY(rq, occ)                                                                     \
    }

void er_launch_wf_begin(const DevScene& S, const WfState& W, uint32_t n_samples, hipStream_t stream);
// ray_log (may be NULL): the launch stores the number of rays it found in its queues there (ER_FLAG_PROFILE)
void er_launch_wf_trace(const DevScene& S, const WfState& W, uint32_t parity, bool count, uint32_t blocks, uint32_t* ray_log, hipStream_t stream);
void er_launch_wf_shade(const DevScene& S, const WfState& W, uint32_t parity, bool count, uint32_t blocks, hipStream_t stream);
