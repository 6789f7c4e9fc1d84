// er_slot_bounce.inc -- er_bounce.inc for a schedule that records its shadow queries in the slot's records (er_wavefront.h) and adds
// their addends at the slot's next step: the wavefront shade kernel and the streaming kernel's shading step.
// In scope besides what er_bounce.inc needs: `slot`, `W`, and ER_SLOT(field, i), the including file's name for field `field` of
// record i.  ER_BOUNCE_FUSE / ER_BOUNCE_MESH are the including site's; the hooks and ER_BOUNCE_MESH are undefined again below.
#define ER_BOUNCE_HDRI_QUERY(sr, self_slot, d_self, cv, co)                                                                  \
    ER_SLOT(sh_o, slot) = make_float4((sr).o.x, (sr).o.y, (sr).o.z, __builtin_bit_cast(float, (int)(self_slot)));            \
    ER_SLOT(sh_d, slot) = make_float4((sr).d.x, (sr).d.y, (sr).d.z, (d_self));                                               \
    ER_SLOT(c_vis, slot) = make_float4((cv).x, (cv).y, (cv).z, 0.0f);                                                        \
    ER_SLOT(c_occ, slot) = make_float4((co).x, (co).y, (co).z, 0.0f)
#define ER_BOUNCE_LIGHT_QUERY(lr, self_slot, limit, lv, lo)                                                                  \
    {   /* the light query of a slot lives in the second half of the shadow records */                                       \
        const uint32_t lq = slot + W.slots;                                                                                  \
        const F3 lv_ = (lv), lo_ = (lo);                                                                                     \
        ER_SLOT(sh_o, lq) = make_float4((lr).o.x, (lr).o.y, (lr).o.z, __builtin_bit_cast(float, (int)(self_slot)));          \
        ER_SLOT(sh_d, lq) = make_float4((lr).d.x, (lr).d.y, (lr).d.z, (limit));                                              \
        ER_SLOT(c_vis, lq) = make_float4(lv_.x, lv_.y, lv_.z, 0.0f);                                                         \
        ER_SLOT(c_occ, lq) = make_float4(lo_.x, lo_.y, lo_.z, 0.0f);                                                         \
    }
#define ER_BOUNCE_FIRST_HIT(n, t, b)                                                                                         \
    ER_SLOT(aov_n, slot) = make_float4((n).x, (n).y, (n).z, 0.0f);                                                           \
    ER_SLOT(aov_t, slot) = make_float4((t).x, (t).y, (t).z, 0.0f);                                                           \
    ER_SLOT(aov_b, slot) = make_float4((b).x, (b).y, (b).z, 0.0f)
#include "er_bounce.inc"
#undef ER_BOUNCE_HDRI_QUERY
#undef ER_BOUNCE_LIGHT_QUERY
#undef ER_BOUNCE_FIRST_HIT
#undef ER_BOUNCE_MESH
