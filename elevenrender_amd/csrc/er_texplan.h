// er_texplan.h -- the texture plan: every layout decision of the texture pool, made once, on the host, from the sizes alone.
// er_render_begin fills the pool on the host by this plan (er_api.cpp begin_textures), er_render_edit fills it on the device
// (er_texstage.hip, from er_api_edit.cpp edit_pool); both read the one plan, so the two layouts can not drift, and tests/test_gpu_edit.py compares the bytes.
// The plan never reads a texel.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../include/eleven_hip.h"
#include "er_device.h"

namespace erh {

struct TexDecl {      // a texture as the plan sees it
    int32_t width, height, channels, filter;
};

struct TexPlan {
    // per texture: 0 as it came, 1 first channel alone, 2 first channel alone to the power 2.2
    std::vector<uint8_t> mode;
    std::vector<DevTex> table;        // per texture, with its offset into the pool
    std::vector<DevFused> fused;      // per material (at least one entry): width 0 = not fused
    DevTex hdri{};                    // the HDRI's texels lie last
    uint64_t pool_floats = 0;         // >= 2^32: the pool can not be addressed (offsets are 32 bits) and nothing may be built
    bool fused_any = false;
};

// The pool in order: the textures in list order, the fused records in material order, the HDRI.
//
// A texture that materials use ONLY for scalar channels -- opacity, roughness, metallic, transmission take `.x` of the fetched value
// (src/kernel.cpp:100-150) -- is kept on the device with its first channel alone: a one-channel fetch returns that value in .x
// (src/Texture.cpp:181-184), the filter's arithmetic on .x is the same, and the pool of C5 (64 x 3 noise textures of 3 channels, two
// of the three used for roughness and metallic) shrinks from 151 MB to 84 MB of the caches it shares with the tree.
// And where such a texture is read UNFILTERED and only as roughness or metallic, what it holds is the value to the power 2.2 that
// generateHitData takes of every fetch (src/kernel.cpp:152-153), computed with the device's own er_pow (er_math.h: one
// implementation, the same bits -- as for the constants of DevScene::mat_pre); DevTex::filter = 2 marks it (fetched like filter 0).
//
// A material whose albedo, roughness and metallic textures have one size and one filter gets them texel by texel in one record of
// five floats (DevFused, er_device.h): one fetch, one cache line and one coordinate computation per hit instead of three.  The
// texel values are what Texture::getValueFromCoordinates returns for each (src/Texture.cpp:172-200); unfiltered, roughness and
// metallic are stored to the power 2.2 as above.  The textures themselves stay where they are for every other use.
inline void er_texture_plan(const TexDecl* tex, size_t ntex, const ErMaterial* mats, size_t nmat, const TexDecl& hdri, TexPlan& P) {
    std::vector<uint8_t> vec_use(ntex, 0), scal_use(ntex, 0), plain_use(ntex, 0);
    auto mark = [&](std::vector<uint8_t>& v, int32_t id) { if (id >= 0 && (size_t)id < v.size()) v[(size_t)id] = 1; };
    for (size_t m = 0; m < nmat; m++) {
        const ErMaterial& M = mats[m];
        mark(vec_use, M.albedo_tex); mark(vec_use, M.emission_tex); mark(vec_use, M.normal_tex);
        mark(scal_use, M.opacity_tex); mark(scal_use, M.roughness_tex); mark(scal_use, M.metallic_tex); mark(scal_use, M.transmission_tex);
        mark(plain_use, M.opacity_tex); mark(plain_use, M.transmission_tex);      // (scalar channels that are NOT raised to a power)
    }
    const char* compact_knob = getenv("ER_TEX_COMPACT");      // (A/B and test knob: 0 = every texture as it came)
    const bool compact = !(compact_knob && atoi(compact_knob) == 0);
    const bool pow_on_host = !getenv("ER_MAT_PRE_ON_DEVICE");
    auto texels = [](const TexDecl& t) { return (uint64_t)std::max(0, t.width) * (uint64_t)std::max(0, t.height); };
    P.mode.assign(ntex, 0);
    P.table.assign(ntex, DevTex{0, 0, 0, 0, 0});
    uint64_t off = 0;
    for (size_t i = 0; i < ntex; i++) {
        const TexDecl& t = tex[i];
        if (compact && t.channels >= 1 && scal_use[i] && !vec_use[i]) {
            const bool powered = t.filter != 1 && !plain_use[i] && pow_on_host;
            if (t.channels > 1 || powered) P.mode[i] = powered ? 2 : 1;
        }
        if (P.mode[i]) {
            P.table[i] = DevTex{t.width, t.height, 1, P.mode[i] == 2 ? 2 : (t.filter == 1 ? 1 : 0), (uint32_t)off};
            off += texels(t);
        } else {
            // (anything but BILINEAR fetches unfiltered, src/Texture.cpp:229-236; 2 is the library's own mark)
            P.table[i] = DevTex{t.width, t.height, t.channels, t.filter == 1 ? 1 : 0, (uint32_t)off};
            off += texels(t) * (uint64_t)std::max(0, t.channels);
        }
    }
    P.fused.assign(std::max<size_t>(1, nmat), DevFused{0, 0, 0, 0});
    P.fused_any = false;
    const char* fuse_knob = getenv("ER_TEX_FUSE");      // (A/B knob; ER_TEX_COMPACT=0 = "every texture as it came" switches this off as well)
    if (compact && !(fuse_knob && atoi(fuse_knob) == 0)) {
        for (size_t m = 0; m < nmat; m++) {
            const ErMaterial& M = mats[m];
            const int32_t ids[3] = {M.albedo_tex, M.roughness_tex, M.metallic_tex};
            bool ok = true;
            for (int32_t id : ids) ok = ok && id >= 0 && (size_t)id < ntex;
            if (!ok) continue;
            const TexDecl &A = tex[(size_t)ids[0]], &R = tex[(size_t)ids[1]], &K = tex[(size_t)ids[2]];
            if (A.width != R.width || A.width != K.width || A.height != R.height || A.height != K.height) continue;
            if ((A.filter == 1) != (R.filter == 1) || (A.filter == 1) != (K.filter == 1)) continue;
            if (A.channels < 1 || R.channels < 1 || K.channels < 1) continue;
            const bool bilinear = A.filter == 1, powered = !bilinear && pow_on_host;
            const uint64_t n = texels(A);
            if (off + 5 * n >= (1ull << 32)) continue;
            P.fused[m] = DevFused{A.width, A.height, bilinear ? 1 : (powered ? 2 : 0), (uint32_t)off};
            P.fused_any = P.fused_any || A.width > 0;
            off += 5 * n;
        }
    }
    P.hdri = DevTex{hdri.width, hdri.height, hdri.channels, hdri.filter, (uint32_t)off};
    P.pool_floats = off + texels(hdri) * (uint64_t)std::max(0, hdri.channels);
}

}  // namespace erh
