// er_stream_host.cpp -- host side of the streaming schedule (ER_FLAG_STREAM; the kernel and its launcher: er_stream.hip): the deal of
// tiles to workgroups, the choice of the kernel's form for a share, the schedule's set-up at er_render_begin, the re-deal of an
// adaptive render, the launches of a call, the status read-back and the adaptation between calls.  All of its state in a scene is
// ErScene::st (er_stream_host.h); er_api.cpp, er_collective.cpp and er_debug_api.cpp reach it through the functions here.
#include <algorithm>
#include <map>

#include "er_scene.h"
#include "../../include/eleven_hip_debug.h"

using namespace erh;

// Which workgroup renders which tiles.  Workgroups b and b + 8 run on the same XCD and share its 4 MB L2 (observed dispatch
// order, MI355X_MICROARCH.md; used for speed only -- any deal gives the same pixels), so the frame is cut into super-tiles of
// edge x edge tiles (8: 64 x 64 pixels; er_render_begin also makes the deal of 16, er_stream.h), every super-tile goes to ONE XCD (the
// one with the fewest tiles so far), the XCDs are then levelled tile by tile, and inside an XCD the
// tiles are dealt round-robin to its workgroups: the camera rays and first bounces that an L2 serves then come from a few
// compact screen regions instead of from every eighth tile of the whole frame.  out[b + k * blocks] = the k-th tile of
// workgroup b, 0xFFFFFFFF = none; returns the largest number of tiles any workgroup got.
uint32_t er_stream_deal_tiles(const uint32_t* owned, uint32_t count, uint32_t tiles_x, uint32_t blocks, bool xcd_aware, std::vector<uint32_t>& out, uint32_t edge) {
    if (edge == 0u) {
        const char* e = getenv("ER_STREAM_SUPER_TILE");      // (A/B knob)
        const int v = e ? atoi(e) : 0;
        edge = v >= 1 ? (uint32_t)v : ER_STREAM_SUPER_TILE_DEFAULT;
    }
    const uint32_t X = (xcd_aware && blocks % 8u == 0u) ? 8u : 1u, per = blocks / X, S8 = edge;
    const uint32_t super_x = (tiles_x + S8 - 1u) / S8;
    std::map<uint32_t, std::vector<uint32_t>> by_super;      // row-major super-tile order; tiles inside keep their row-major order
    for (uint32_t i = 0; i < count; i++) {
        const uint32_t tx = owned[i] % tiles_x, ty = owned[i] / tiles_x;
        by_super[X == 1u ? 0u : (ty / S8) * super_x + tx / S8].push_back(owned[i]);
    }
    std::vector<std::vector<uint32_t>> seq(X);
    for (auto& kv : by_super) {
        uint32_t best = 0;
        for (uint32_t x = 1; x < X; x++) if (seq[x].size() < seq[best].size()) best = x;
        seq[best].insert(seq[best].end(), kv.second.begin(), kv.second.end());
    }
    // Whole super-tiles leave the XCDs up to one super-tile apart (1.6 % of an XCD's share of a 1080p frame at the default edge, 6 % at
    // 16) and a launch lasts as long as its fullest XCD: level them tile by tile -- the tail of the fullest XCD's last super-tile goes
    // to the emptiest one -- until no two differ by more than a tile (tests/test_abi_cpu.py; within noise on the soup frames,
    // profiles/r04_sweep_super_tile.log: what a larger super-tile loses on a frame of uneven cost is the CONTENT of its XCDs' shares).
    const char* lv = getenv("ER_STREAM_LEVEL_XCDS");      // (A/B knob)
    for (; !(lv && atoi(lv) == 0);) {
        uint32_t hi = 0, lo = 0;
        for (uint32_t x = 1; x < X; x++) {
            if (seq[x].size() > seq[hi].size()) hi = x;
            if (seq[x].size() < seq[lo].size()) lo = x;
        }
        const size_t diff = seq[hi].size() - seq[lo].size();
        if (diff <= 1u) break;
        const size_t n = diff / 2u;
        seq[lo].insert(seq[lo].end(), seq[hi].end() - (ptrdiff_t)n, seq[hi].end());
        seq[hi].resize(seq[hi].size() - n);
    }
    uint32_t maxk = 0;
    for (uint32_t x = 0; x < X; x++) maxk = std::max<uint32_t>(maxk, (uint32_t)((seq[x].size() + per - 1u) / per));
    out.assign((size_t)blocks * maxk, 0xFFFFFFFFu);
    for (uint32_t x = 0; x < X; x++)
        for (size_t sidx = 0; sidx < seq[x].size(); sidx++) {
            const uint32_t j = (uint32_t)(sidx % per), k = (uint32_t)(sidx / per), b = j * X + x;      // b % X == x: the XCD
            out[(size_t)b + (size_t)k * blocks] = seq[x][sidx];
        }
    return maxk;
}

// The same deal levelled by COUNTED cost.  The count deal gives every workgroup the same positions of every super-tile, and a frame has
// structure: on the C2 frame the workgroups' shares of the counted bounce-loop iterations are 0.964 ... 1.040 of their mean, the same
// workgroups heavy in every sample (NOTEBOOK.md), and a launch lasts as long as its slowest workgroup.  Two stages, both on integers (the
// same costs give the same bytes):
//   the XCDs -- while the costliest exceeds the cheapest by more than twice the cost of the costliest one's LAST tile, that tile goes to
//   the end of the cheapest one's sequence: as in the count levelling above what moves is the edge of a super-tile, the map of
//   super-tiles to XCDs (L2 locality) otherwise stays;
//   inside each XCD -- its tiles by (cost descending, tile ascending), each to the workgroup with the smallest summed cost that has
//   fewer than `cap` tiles (ties: the lower workgroup), a workgroup's tiles then in ascending order.  The greedy rule leaves the largest
//   workgroup within one tile's cost of the XCD's mean wherever the cap does not bind.
// cap = cells of a pixel ring / 64: the rings and their tickets do not grow.  A total cost of 0, or a deal that does not fit the cap,
// comes back as it was.  (tiles_x: the layout's, kept in the signature beside er_stream_deal_tiles'; the levelling needs no geometry.)
uint32_t er_stream_level_by_cost(const std::vector<uint32_t>& deal, uint32_t tiles_x, uint32_t blocks, const uint32_t* cost, size_t cost_n, uint32_t cap, std::vector<uint32_t>& out) {
    (void)tiles_x;
    const uint32_t NONE = 0xFFFFFFFFu;
    const uint32_t rows = blocks ? (uint32_t)(deal.size() / blocks) : 0u;
    auto keep = [&]() { out = deal; return rows; };
    if (!blocks || !rows || !cap) return keep();
    const uint32_t X = blocks % 8u == 0u ? 8u : 1u, per = blocks / X;
    auto c_of = [&](uint32_t t) -> uint64_t { return (cost && t < cost_n) ? cost[t] : 0u; };
    // the XCDs' sequences in the order er_stream_deal_tiles dealt them: entry j + k * per of XCD x is the k-th tile of workgroup j * X + x
    std::vector<std::vector<uint32_t>> seq(X);
    std::vector<uint64_t> sum(X, 0);
    uint64_t total = 0;
    for (uint32_t k = 0; k < rows; k++)
        for (uint32_t j = 0; j < per; j++)
            for (uint32_t x = 0; x < X; x++) {
                const uint32_t t = deal[(size_t)(j * X + x) + (size_t)k * blocks];
                if (t == NONE) continue;
                seq[x].push_back(t); sum[x] += c_of(t); total += c_of(t);
            }
    if (total == 0) return keep();
    for (uint32_t x = 0; x < X; x++) if (seq[x].size() > (size_t)per * cap) return keep();
    for (;;) {      // (every move lowers the sum of the XCDs' squared costs: it ends)
        uint32_t hi = 0, lo = 0;
        for (uint32_t x = 1; x < X; x++) {
            if (sum[x] > sum[hi]) hi = x;
            if (sum[x] < sum[lo]) lo = x;
        }
        if (hi == lo || seq[hi].empty() || seq[lo].size() >= (size_t)per * cap) break;
        const uint32_t t = seq[hi].back();
        const uint64_t c = c_of(t);
        if (c == 0 || sum[hi] - sum[lo] <= 2u * c) break;
        seq[hi].pop_back(); seq[lo].push_back(t);
        sum[hi] -= c; sum[lo] += c;
    }
    std::vector<std::vector<uint32_t>> mine(blocks);
    std::vector<uint64_t> load(per);
    uint32_t most = 0;
    for (uint32_t x = 0; x < X; x++) {
        std::vector<uint32_t>& q = seq[x];
        std::sort(q.begin(), q.end(), [&](uint32_t a, uint32_t b) { const uint64_t ca = c_of(a), cb = c_of(b); return ca != cb ? ca > cb : a < b; });
        std::fill(load.begin(), load.end(), 0);
        for (uint32_t t : q) {
            uint32_t best = per;
            for (uint32_t j = 0; j < per; j++)
                if (mine[(size_t)j * X + x].size() < cap && (best == per || load[j] < load[best])) best = j;
            if (best == per) return keep();      // (cannot happen: the XCD holds at most per * cap tiles)
            mine[(size_t)best * X + x].push_back(t);
            load[best] += c_of(t);
        }
    }
    for (auto& m : mine) { std::sort(m.begin(), m.end()); most = std::max<uint32_t>(most, (uint32_t)m.size()); }
    out.assign((size_t)blocks * most, NONE);
    for (uint32_t b = 0; b < blocks; b++)
        for (size_t k = 0; k < mine[b].size(); k++) out[(size_t)b + k * blocks] = mine[b][k];
    return most;
}

bool stream_xcd_aware(size_t owned_tiles, uint32_t blocks) {
    const char* xe = getenv("ER_STREAM_XCD_TILES");        // A/B knob: 0 = tiles dealt round-robin to the workgroups (round 2)
    // (a share with no more pixels than slots -- an eighth of a 1080p frame -- has nothing waiting in its pixel rings; there the
    // plain round-robin deal balances a little better: 1.392 vs 1.41 ms per pass, profiles/r03_ab_sim_world8_knobs.log)
    return xe ? atoi(xe) != 0 : owned_tiles * 64 > (size_t)blocks * ER_STREAM_SLOTS;
}

StreamDeal stream_deal_owned(const std::vector<uint32_t>& owned, uint32_t tiles_x, uint32_t cus) {
    StreamDeal d;
    d.most = er_stream_deal_tiles(owned.data(), (uint32_t)owned.size(), tiles_x, cus, stream_xcd_aware(owned.size(), cus), d.tiles);
    return d;
}

// (er_render_begin for the owned share; an adaptive render again for every new active share, within the buffers begin made)
StreamForm stream_choose_form(size_t tiles, uint32_t blocks, bool light_query, uint32_t tri_count, uint32_t flags) {
    StreamForm f;
    // The split between tracer and shader waves (shader waves at issue priority 1; finished and escaped paths handled in batches
    // of their own, er_stream.hip).  Round 2: 10 + 6, round 3: 12 + 4 (11 + 5 with the point-light extension, whose shading
    // step is a third longer); since round 4's shorter shading step:
    // 13 tracer + 3 shader waves where the shading step is at its cheapest -- plain materials, a scene that lives in the caches
    // (C2: 1 787 vs 1 715 Msamples/s at 12 + 4) -- and 12 + 4 where it costs more: textured materials (C5 without lights: 1 560 vs
    // 1 489 at 13 + 3), point lights (C5: 1 350 vs 1 234), or a scene beyond the Infinity Cache (C4, 10 M triangles: 1 562 vs 1 483)
    // (profiles/r04_sweep_split_after_shader_diet.log).  That is the split to begin with; after every completed call it follows how
    // full the tracer lanes were (stream_adapt: a scene of another kind that starves 13 tracers gets 12 after its first call).
    // (textured materials started at 12 + 4 until their textures were fused / pre-powered / one-channel, er_render_begin: C5 without
    // lights now 1 712 vs 1 640 at 12 + 4; a textured scene whose shading step is still too long for 13 tracers reads < 0.85 full lanes
    // after its first call and gets 12)
    // (swept again after er_bounce.inc stopped tracing the shadow queries of dead paths -- a shading step then yields 1.06 rays instead of
    // 1.22 on C2 and the tracer lanes read 0.88 instead of 0.91 at 13 + 3 --: the same splits win, C2 2 026 vs 1 989 at 12 + 4, C5 without
    // lights 1 925 vs 1 881, C5 with lights 1 771 at 12 + 4 vs 1 587, C4 1 784 vs 1 661; profiles/equal_queries_ab.log)
    const uint32_t large_tracers = (light_query || tri_count > 4000000u) ? 12u : 13u;
    f.tracers = large_tracers;
    // A workgroup that owns hardly more pixels than it has slots (an eighth of a 1080p frame: 1 012 pixels per CU) cannot fill 12 tracer
    // waves -- a pixel's samples are one RNG stream, so pixels in flight are all the parallelism there is -- and runs faster as 9 tracer +
    // 3 shader waves of 168 registers (the shading step then spills 34 registers instead of 111 and three shader waves serve what four
    // did): 1.23 vs 1.35 ms per pass at 1/8 (1 012 pixels per CU); at 1/6 (1 350 pixels) 16 waves are ahead again, 1.43 vs 1.47 (profiles/r04_sweep_small_shares.log)
    f.waves = 16;
    const size_t px_per_cu = tiles * 64 / std::max<uint32_t>(1u, blocks);
    // (round 6, profiles/r06_ab_long_pixels_and_split.log: with the shading step as short as it has become two shader waves serve ten tracers where
    // the slots are nearly all taken -- 1/8 ... 1/11 of the C2 frame 4.5 ... 1.5 % faster, C5's 1/8 share 1 ... 3 % -- and from 1/12 down 9 + 3 is ahead by 2 %)
    const uint32_t small_tracers = px_per_cu > ER_STREAM_TEN_TRACERS_SHARE ? 10u : 9u;
    if (px_per_cu <= ER_STREAM_SMALL_SHARE) { f.waves = 12; f.tracers = small_tracers; }
    // the lane occupancy says something about the balance of the two roles only where pixels are plentiful: a share of a few
    // pixels per slot cannot fill the lanes whatever the split (an eighth of a 1080p frame: 0.59 at the fastest split)
    // (nor in the instrumented kernel of ER_FLAG_COUNTERS, whose slower tracer loop shifts the balance)
    f.adapt = px_per_cu >= 4u * ER_STREAM_SLOTS && !(flags & ER_FLAG_COUNTERS);
    f.keep = px_per_cu <= ER_STREAM_KEEP_SHARE;      // (er_stream.hip s_front)
    f.spec = px_per_cu <= ER_STREAM_SPEC_SHARE;      // few pixels per slot: slots fall free, speculative samples can use them (er_stream.hip)
    if (const char* e = getenv("ER_STREAM_SPEC_FORM")) f.spec = atoi(e) != 0;      // A/B knob
    if (const char* e = getenv("ER_STREAM_KEEP")) f.keep = atoi(e) != 0;           // A/B knob
    if (const char* e = getenv("ER_STREAM_WAVES")) { f.waves = atoi(e) == 12 ? 12 : 16; f.tracers = f.waves == 12 ? small_tracers : large_tracers; }   // A/B knob
    if (const char* e = getenv("ER_STREAM_TRACERS")) { f.tracers = (uint32_t)std::min(13, std::max(1, atoi(e))); f.adapt = false; }   // tuning knob: fixed split
    if (const char* e = getenv("ER_STREAM_ADAPT")) f.adapt = atoi(e) != 0;
    return f;
}

// the form for a share of `tiles` tiles, and the adaptation of its split starts over (the readings of a render go on: begin zeroes them)
static void stream_set_form(ErScene* s, size_t tiles) {
    StreamHost& st = s->st;
    st.form = stream_choose_form(tiles, st.blocks, st.lights, s->tri_count, s->params.flags);
    st.tracers_start = st.form.tracers; st.low_streak = 0; st.up_budget = 1;
}

// A decision between the two deals that is still open is closed and the kernel stops counting -- the scene descriptor it reads loses the
// pointer (ordered on the stream before the next launch) -- and the host's copies of the large deal and of the deal to level go.
static hipError_t stream_drop_pending_deal(ErScene* s) {
    s->st.deal_pending = false;
    s->st.counting = false;
    s->dev.tile_cost = s->ad_dev.tile_cost = nullptr;
    s->st.deal_large.clear(); s->st.deal_large.shrink_to_fit();
    s->st.deal_base.clear(); s->st.deal_base.shrink_to_fit();
    return hipMemcpyAsync(s->d_dev.p, &s->dev, sizeof(DevScene), hipMemcpyHostToDevice, s->stream);
}

int stream_begin(ErScene* s, const std::vector<uint32_t>& owned, StreamDeal& deal, uint32_t cus, bool light_query) {
    // one workgroup per CU with ER_STREAM_SLOTS slots of the wavefront schedule's records each
    StreamHost& st = s->st;
    int rc;
    st.blocks = cus;
    st.lights = light_query;
    stream_set_form(s, owned.size());
    st.readings = 0;
    const size_t slots = (size_t)st.blocks * ER_STREAM_SLOTS, npx = (size_t)s->x_res * s->y_res;
    if ((rc = upload(s->d_wf4, nullptr, slots * er_stream_record_bytes(light_query) / sizeof(float4), s->stream)) != ER_OK) return rc;
    const size_t ctl_words = ER_STREAM_CTL_LEAD + er_stream_ctl_words(st.blocks);
    if ((rc = upload(s->d_wf1, nullptr, ctl_words, s->stream)) != ER_OK) return rc;       // the control words (er_stream.h ErStreamCtl)
    if ((rc = upload(s->d_spill, nullptr, er_stream_spill_entries(st.blocks), s->stream)) != ER_OK) return rc;
    st.ctl = s->d_wf1.p;
    HIP_TRY(hipMemsetAsync(st.ctl, 0, ctl_words * sizeof(uint32_t), s->stream));
    st.spec[0] = st.spec[1] = st.spec[2] = 0;
    st.launch_start = st.launch_end = 0; st.wg_end.clear();
    // the workgroups' pixel rings: (pixel, samples left) entries, one per pixel of the workgroup's share
    // (capacity rounded up to a power of two: positions are monotonic 32-bit counters and may wrap)
    // (no minimum beyond one tile: a producer that comes round to a cell whose entry has not been read yet waits for its
    // reader, er_ring.h -- round 2 relied on "a lap of >= 4096 cells takes longer than a read")
    const bool xcd_aware = stream_xcd_aware(owned.size(), st.blocks);
    const uint32_t tiles_x = s->tiles_x();
    uint32_t most = deal.most;
    st.deal_off = 0; st.deal_n = (uint32_t)deal.tiles.size();
    st.deal_alt_off = 0; st.deal_alt_n = 0;
    st.deal_base_off = 0; st.deal_lvl_off = 0; st.deal_lvl_cap = 0; st.deal_levelled = false;
    st.counting = false;
    st.deal_base.clear(); st.cost_host.clear();
    st.deal_host = deal.tiles;
    st.xcd_spread = -1.0;
    // Larger screen regions per XCD are faster where a frame's cost is even and slower where it is not (er_stream.h), and only the run
    // can tell which.  With the knob unset a render STARTS on the default deal -- it spreads any frame's cost over the XCDs -- and keeps
    // the deal of ER_STREAM_SUPER_TILE_LARGE beside it in d_deal; during the first call the kernel adds every finished path's length to
    // its tile's sum (DevScene::tile_cost: counted work, not a measured time), and stream_adapt takes the large regions, for good,
    // if under THAT deal the XCDs' shares of the counted work are within ER_STREAM_COST_SPREAD_MAX of each other.  (Round 4 started
    // on the large deal and fell back on the XCDs' measured finish times: an uneven frame paid 8-18 % for its first call, and the
    // decision -- and the test of it -- hung on clocks.)
    const char* adapt_knob = getenv("ER_STREAM_ADAPT");
    st.deal_pending = false;
    st.deal_large.clear();
    st.d_tile_cost.release();
    if (xcd_aware && st.blocks % 8u == 0u && owned.size() * 64 / st.blocks >= ER_STREAM_SLOTS * 3u / 2u && !(s->params.flags & ER_FLAG_COUNTERS) &&      // (a half / a quarter of a 1080p frame: +1.2 % / +0.7 %)
        !getenv("ER_STREAM_SUPER_TILE") && !(adapt_knob && atoi(adapt_knob) == 0)) {
        std::vector<uint32_t> large;
        const uint32_t most_large = er_stream_deal_tiles(owned.data(), (uint32_t)owned.size(), tiles_x, st.blocks, xcd_aware, large, ER_STREAM_SUPER_TILE_LARGE);
        if ((size_t)most_large * 64u <= ER_STREAM_MAX_RING) {      // (levelled, the two deals have the same largest share; never let the optional one fail the call)
            st.deal_alt_off = (uint32_t)deal.tiles.size(); st.deal_alt_n = (uint32_t)large.size();
            deal.tiles.insert(deal.tiles.end(), large.begin(), large.end());
            most = std::max(most, most_large);
            st.deal_large.swap(large);
            const size_t n_tiles = (size_t)tiles_x * s->tiles_y();
            if ((rc = upload(st.d_tile_cost, nullptr, n_tiles, s->stream)) != ER_OK) return rc;
            HIP_TRY(hipMemsetAsync(st.d_tile_cost.p, 0, n_tiles * sizeof(uint32_t), s->stream));
            st.deal_pending = st.counting = true;
        }
    }
    if ((rc = upload(st.d_px_draws, nullptr, npx, s->stream)) != ER_OK) return rc;
    HIP_TRY(hipMemsetAsync(st.d_px_draws.p, 0, npx * sizeof(uint32_t), s->stream));
    if (s->x_res > 65535u || s->y_res > 65535u)
        return fail(ER_ERR_INVALID_ARG, "er_render_begin: ER_FLAG_STREAM carries a pixel as x | y << 16: frames up to 65535 x 65535; use ER_FLAG_WAVEFRONT (the automatic choice does)");
    st.ring_cap = 64u;
    while (st.ring_cap < most * 64u) st.ring_cap <<= 1;
    if (st.ring_cap > ER_STREAM_MAX_RING)
        return fail(ER_ERR_INVALID_ARG, "er_render_begin: ER_FLAG_STREAM serves at most " + std::to_string((size_t)ER_STREAM_MAX_RING * st.blocks) +
                                            " owned pixels per rank; use ER_FLAG_WAVEFRONT (the automatic choice does)");
    if ((rc = upload(st.d_ticket, nullptr, (size_t)st.blocks * (size_t)st.ring_cap * 2, s->stream)) != ER_OK) return rc;
    // (behind the two deals: room for the one taken, levelled by counted cost -- at most ring_cap / 64 tiles per workgroup, stream_adapt)
    if (st.counting) { st.deal_lvl_off = (uint32_t)deal.tiles.size(); st.deal_lvl_cap = st.blocks * (st.ring_cap / 64u); }
    if ((rc = upload(st.d_deal, nullptr, deal.tiles.size() + st.deal_lvl_cap, s->stream)) != ER_OK) return rc;
    if (!deal.tiles.empty()) HIP_TRY(hipMemcpyAsync(st.d_deal.p, deal.tiles.data(), deal.tiles.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
    return ER_OK;
}

int stream_redeal(ErScene* s) {
    StreamHost& st = s->st;
    // (a decision between the two deals still pending -- calls of one sample each until now -- is dropped: the default deal stays; the
    // large regions, if already taken, stay taken for the new share)
    // (nor does a deal levelled by counted cost survive: the new share is dealt by count, and the counting stops)
    const bool large = st.large_deal_in_use();
    if (st.deal_pending || st.counting) HIP_TRY(stream_drop_pending_deal(s));
    const uint32_t count = (uint32_t)s->ad_active.size(), tiles_x = s->tiles_x();
    std::vector<uint32_t> deal;
    uint32_t most = er_stream_deal_tiles(s->ad_active.data(), count, tiles_x, st.blocks, stream_xcd_aware(count, st.blocks), deal, large ? ER_STREAM_SUPER_TILE_LARGE : 0u);
    // (whole super-tiles can leave one workgroup more tiles of a small share than it had of the owned one; the round-robin deal never
    // does: ceil(count / blocks) <= ceil(owned / blocks) <= the owned share's largest, which the rings were sized for)
    if ((size_t)most * 64u > st.ring_cap) most = er_stream_deal_tiles(s->ad_active.data(), count, tiles_x, st.blocks, false, deal);
    if ((size_t)most * 64u > st.ring_cap) return fail(ER_ERR_STATE, "er_render_samples: the active tiles do not fit the pixel rings");
    int rc;
    if ((rc = upload(st.d_deal, deal.data(), deal.size(), s->stream)) != ER_OK) return rc;
    st.deal_off = 0; st.deal_n = (uint32_t)deal.size();
    st.deal_alt_off = 0; st.deal_alt_n = 0;
    st.deal_base_off = 0; st.deal_lvl_off = 0; st.deal_lvl_cap = 0; st.deal_levelled = false;
    st.deal_host = deal;
    stream_set_form(s, count);
    HIP_TRY(hipStreamSynchronize(s->stream));      // (`deal` goes out of scope)
    return ER_OK;
}

static int stream_launch(ErScene* s, uint32_t k) {
    StreamHost& st = s->st;
    HIP_TRY(hipMemsetAsync(st.status() + ER_SC_ITERS, 0, (er_stream_ctl_words(st.blocks) - ER_SC_ITERS) * sizeof(uint32_t), s->stream));      // the call's lane-occupancy counts, its end per XCD and per workgroup, its speculation counts ...
    HIP_TRY(hipMemsetAsync(st.status() + ER_SC_START, 0xFF, 2 * sizeof(uint32_t), s->stream));                            // ... and its start (a minimum)
    if (k > 0) st.launches++;
    ErStreamLaunch L;
    L.S = &s->dev; L.S_dev = s->d_dev.p;
    L.records = s->d_wf4.p; L.slots = st.blocks * ER_STREAM_SLOTS; L.lights = st.lights;
    L.spill = s->d_spill.p;
    L.deal = st.d_deal.p + st.deal_off; L.deal_count = st.deal_n;
    L.ring = st.d_ticket.p; L.ring_cap = st.ring_cap;
    L.status = st.status();
    L.n_samples = k;
    L.count = (s->params.flags & ER_FLAG_COUNTERS) != 0;
    L.blocks = st.blocks; L.tracers = st.form.tracers; L.waves = st.form.waves; L.spec = st.form.spec; L.keep = st.form.keep;
    L.stream = s->stream;
    er_launch_stream(L);
    return ER_OK;
}

int stream_enqueue(ErScene* s, uint32_t n) {
    StreamHost& st = s->st;
    // Round 6: a render that is ONE call must get the deal its frame deserves too.  While the deal is undecided, the first call's
    // first sample is a launch of its own: the kernel counts that pass's path lengths per tile (a count of work, the same on every
    // run), the library decides -- and stops the counting -- and the other n - 1 samples run on the deal decided.  Until round 6 the
    // decision came after the first CALL, so a host that issued one er_render_samples(256) never left the default deal (C2 -1.5 ... -4 %,
    // C4 -3 ... -5.7 %) and `bench.py --warmup 0` measured another kernel configuration than `--warmup 5`.  Cost: one more launch per
    // render (~0.8 ms) and a host wait of one sample pass inside this call, once; the image does not depend on the deal.
    static const bool split_first = [] { const char* e = getenv("ER_STREAM_SPLIT_FIRST"); return !(e && atoi(e) == 0); }();      // (A/B knob)
    int rc;
    if (st.deal_pending && n >= 2u && split_first) {
        if ((rc = stream_launch(s, 1u)) != ER_OK) return rc;
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s->stream));
        if ((rc = er_scene_stream_status(s, "er_render_samples")) != ER_OK) return rc;
        st.probe_launch = true;      // (a one-pass launch is no reading of the tracer lanes' occupancy: only the deal is decided on it)
        stream_adapt(s);
        st.probe_launch = false;
        n -= 1u;
    }
    return stream_launch(s, n);
}

// The streaming kernel's waves give up instead of spinning forever if their workgroup makes no progress (er_stream.hip) and
// say so in a status word.  Called with the scene's stream idle (after a wait or a read-back): an unfinished call must not pass
// for a finished one.  The word stays set until the next er_render_begin.
int er_scene_stream_status(ErScene* s, const char* who) {
    StreamHost& st = s->st;
    if (!(s->params.flags & ER_FLAG_STREAM) || !st.ctl) return ER_OK;
    std::vector<uint32_t> w(er_stream_ctl_words(st.blocks), 0u);
    HIP_TRY(hipMemcpy(w.data(), st.status(), w.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (st.spec_seen != st.launches) {      // (once per launch: a read-back after the same launch finds the same words)
        st.spec_seen = st.launches;
        for (int k = 0; k < 3; k++) st.spec[k] += w[ER_SC_SPEC + k];
    }
    if (w[ER_SC_STATUS] != 0)
        return fail(ER_ERR_STATE, std::string(who) + ": the streaming schedule stopped without finishing (watchdog status " + std::to_string(w[ER_SC_STATUS]) + "); the planes are incomplete");
    auto u64 = [&](uint32_t i) { return (unsigned long long)w[i] | ((unsigned long long)w[i + 1] << 32); };
    const unsigned long long iters = u64(ER_SC_ITERS), busy = u64(ER_SC_BUSY);
    st.busy = iters ? (double)busy / (64.0 * (double)iters) : 0.0;
    // how far apart the XCDs finished, as a share of the launch (100 MHz ticks; a launch under 2 ms says nothing: start-up and tail)
    const unsigned long long t0 = u64(ER_SC_START);
    unsigned long long lo = ~0ull, hi = 0;
    for (uint32_t x = 0; x < 8; x++) { const unsigned long long e = u64(ER_SC_END + 2 * x); lo = std::min(lo, e); hi = std::max(hi, e); }
    st.xcd_spread = (t0 != ~0ull && lo > t0 && hi - t0 >= 200000ull) ? (double)(hi - lo) / (double)(hi - t0) : -1.0;
    st.launch_ms = (t0 != ~0ull && hi > t0) ? (double)(hi - t0) * 1e-5 : 0.0;
    // ... and every workgroup's end (er_debug_stream_balance, ER_STREAM_VERBOSE: printed and logged, never acted on)
    st.launch_start = (t0 != ~0ull && hi > t0) ? t0 : 0u; st.launch_end = st.launch_start ? hi : 0u;
    st.wg_end.assign(st.blocks, 0u);
    for (uint32_t b = 0; b < st.blocks; b++) st.wg_end[b] = u64(ER_SC_WG_END + 2 * b);
    return ER_OK;
}

// per workgroup of the deal in use: tiles, counted cost (the tile costs last read), end stamp minus launch start of the last completed launch
void stream_balance(const ErScene* s, std::vector<uint32_t>& wg_tiles, std::vector<uint64_t>& wg_cost, std::vector<uint64_t>& wg_ticks) {
    const StreamHost& st = s->st;
    wg_tiles.assign(st.blocks, 0u); wg_cost.assign(st.blocks, 0u); wg_ticks.assign(st.blocks, 0u);
    for (size_t i = 0; i < st.deal_host.size() && st.blocks; i++) {
        const uint32_t t = st.deal_host[i];
        if (t == 0xFFFFFFFFu) continue;
        wg_tiles[i % st.blocks]++;
        if (t < st.cost_host.size()) wg_cost[i % st.blocks] += st.cost_host[t];
    }
    for (uint32_t b = 0; b < st.blocks && b < st.wg_end.size(); b++)
        if (st.launch_start && st.wg_end[b] > st.launch_start) wg_ticks[b] = st.wg_end[b] - st.launch_start;
}

// ER_STREAM_VERBOSE: how evenly the launch just completed ended and how evenly its deal spread the counted work -- over the workgroups that
// own a tile.  S = (latest end - mean end) / (latest end - launch start): the idle tail, what a better deal could win at most.  Measured
// times: printed, nothing is decided on them.
static void stream_print_balance(const ErScene* s) {
    const StreamHost& st = s->st;
    std::vector<uint32_t> tiles; std::vector<uint64_t> cost, ticks;
    stream_balance(s, tiles, cost, ticks);
    double t_sum = 0, t_max = 0, t_min = 0, c_sum = 0, c_max = 0, c_min = 0;
    uint32_t n = 0, n_max = 0, n_min = 0;
    for (uint32_t b = 0; b < st.blocks; b++) {
        if (!tiles[b] || !ticks[b]) continue;
        const double t = (double)ticks[b], c = (double)cost[b];
        if (!n) { t_max = t_min = t; c_max = c_min = c; n_max = n_min = tiles[b]; }
        t_sum += t; t_max = std::max(t_max, t); t_min = std::min(t_min, t);
        c_sum += c; c_max = std::max(c_max, c); c_min = std::min(c_min, c);
        n_max = std::max(n_max, tiles[b]); n_min = std::min(n_min, tiles[b]);
        n++;
    }
    if (!n || t_sum <= 0) return;
    const double t_mean = t_sum / n, c_mean = c_sum / n;
    fprintf(stderr, "[er_stream] workgroups of a launch of %.3f ms: finished max/mean %.4f min/mean %.4f, idle tail S %.4f", t_max * 1e-5, t_max / t_mean, t_min / t_mean, (t_max - t_mean) / t_max);
    if (c_mean > 0) fprintf(stderr, "; counted cost max/mean %.4f min/mean %.4f", c_max / c_mean, c_min / c_mean);
    fprintf(stderr, " (%s deal, %u ... %u tiles; measured times: printed, nothing is decided on them)\n", st.deal_levelled ? "cost-levelled" : "count", n_min, n_max);
}

// The two roles of the streaming kernel feed each other, and which one is short depends on the scene: how long a ray's traversal is
// against how long its shading step is.  What the tracers' lanes say after a call (counted by the kernel itself, two scalar
// operations per iteration): clearly not full = the shader waves cannot produce rays fast enough, and one tracer wave becomes a
// shader wave for the next call.  Measured with the product kernel (profiles/r04_sweep_split_after_shader_diet.log): C2 0.89-0.90 full
// at 13 + 3 (its best split); C4 0.81-0.85 at 13 + 3 and 0.92 at 12 + 4 (its best); C5 with lights 0.75 at 13 + 3, 0.90 at 12 + 4 (its
// best).  Lanes that ARE full say little (C4 looks alike at 12 + 4 and 11 + 5), so the split moves down: one wave after TWO
// consecutive calls whose lanes were under 0.85 full, down to 10 + 6 (7 + 5 of 12 waves).  A call shorter than ER_STREAM_ADAPT_MIN_MS
// of device time is not a reading at all (its lanes are mostly ramp-up and tail: a 1-spp preview would otherwise walk the split
// down for good), and ONE step back up is allowed per render when a later call reads above 0.93 (a demotion caused by two
// unrepresentative calls is undone; a second demotion after that stays).  The image does not depend on the split.
void stream_adapt(ErScene* s) {
    StreamHost& st = s->st;
    if (!(s->params.flags & ER_FLAG_STREAM)) return;
    const bool verbose = getenv("ER_STREAM_VERBOSE") != nullptr;      // (read per call: a test turns it on for one render)
    if (st.adapted == st.launches) return;                            // (a second er_wait after the same launch: its measurements have been used)
    st.adapted = st.launches;
    if (verbose && !st.form.adapt) fprintf(stderr, "[er_stream] tracer lanes %.3f full at %u + %u waves (fixed split)\n", st.busy, st.form.tracers, st.form.waves - st.form.tracers);
    // the deal: large screen regions per XCD if the XCDs' shares of the COUNTED work of the first call are alike under them (er_stream.h,
    // stream_begin).  Decided once, from counts: the same decision on every run of the same frame.
    const bool counted = st.deal_pending || st.counting;
    bool have_cost = false;
    if (counted) {
        std::vector<uint32_t> cost(st.d_tile_cost.n);
        have_cost = hipMemcpy(cost.data(), st.d_tile_cost.p, cost.size() * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess;
        if (have_cost) st.cost_host.swap(cost);
    }
    if (verbose) stream_print_balance(s);      // (the launch just completed: the deal it ran on, the costs counted up to its end)
    if (st.deal_pending) {
        const std::vector<uint32_t>& cost = st.cost_host;
        if (have_cost) {
            double x[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            const std::vector<uint32_t>& L = st.deal_large;
            for (size_t i = 0; i < L.size(); i++)
                if (L[i] != 0xFFFFFFFFu && L[i] < cost.size()) x[(i % st.blocks) % 8u] += (double)cost[L[i]];      // entry b + k * blocks belongs to workgroup b, XCD b % 8
            double lo = x[0], hi = x[0], sum = 0;
            for (double v : x) { lo = std::min(lo, v); hi = std::max(hi, v); sum += v; }
            const double spread = sum > 0 ? (hi - lo) / (sum / 8.0) : 0.0;
            const char* lim_env = getenv("ER_STREAM_COST_SPREAD_MAX");      // (test knob, read per decision: 0 keeps the default deal, a large value takes the large one)
            const double limit = lim_env ? atof(lim_env) : (double)ER_STREAM_COST_SPREAD_MAX;
            const bool take = sum > 0 && spread <= limit;
            st.cost_spread = spread;
            if (verbose) fprintf(stderr, "[er_stream] counted work of the XCDs' shares on super-tiles of %u: %.4f of the mean apart (limit %.4f) -> %s\n", (unsigned)ER_STREAM_SUPER_TILE_LARGE, spread,
                                 limit, take ? "large regions" : "the default deal stays");
            if (take) { st.deal_off = st.deal_base_off = st.deal_alt_off; st.deal_n = st.deal_alt_n; st.deal_host = st.deal_large; }
        }
        st.deal_pending = false;
        st.deal_base = st.deal_host;      // (what the counted cost then levels)
        st.deal_large.clear(); st.deal_large.shrink_to_fit();
    }
    // The deal taken, levelled by the counted cost (er_stream_level_by_cost): after the render's first sample on that sample's counts, and
    // once more when the first CALL has completed on all of its samples' (a one-sample estimate carries ~0.5 % of noise per workgroup, four
    // samples half of that); then the counting stops.  ER_STREAM_COST_LEVEL=0 (A/B knob, read per decision): the count deal stays and the
    // counting stops with the decision.  Decided from counts alone: the same deal on every run of the same frame.
    if (counted) {
        const char* lv = getenv("ER_STREAM_COST_LEVEL");
        const bool level = !(lv && atoi(lv) == 0) && have_cost && st.deal_lvl_cap != 0u && !st.deal_base.empty();
        if (level) {
            std::vector<uint32_t> lvl;
            er_stream_level_by_cost(st.deal_base, s->tiles_x(), st.blocks, st.cost_host.data(), st.cost_host.size(), st.ring_cap / 64u, lvl);
            if (lvl == st.deal_base) {      // (nothing to level: the deal taken is in use)
                st.deal_off = st.deal_base_off; st.deal_n = (uint32_t)st.deal_base.size(); st.deal_levelled = false;
                st.deal_host = st.deal_base;
            } else if (lvl.size() <= st.deal_lvl_cap &&
                       hipMemcpyAsync(st.d_deal.p + st.deal_lvl_off, lvl.data(), lvl.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream) == hipSuccess) {
                (void)hipStreamSynchronize(s->stream);      // (`lvl` is pageable memory: the copy has left it)
                st.deal_off = st.deal_lvl_off; st.deal_n = (uint32_t)lvl.size(); st.deal_levelled = true;
                st.deal_host.swap(lvl);
            }
        }
        if (!level || !st.probe_launch) (void)stream_drop_pending_deal(s);
        (void)hipStreamSynchronize(s->stream);
    }
    if (verbose && st.xcd_spread >= 0.0)
        fprintf(stderr, "[er_stream] XCDs finished %.3f of the launch apart (a measured time: printed, nothing is decided on it)\n", st.xcd_spread);
    if (!st.form.adapt || st.busy <= 0.0 || st.probe_launch) return;
    const uint32_t lo = st.form.waves == 12 ? 7u : 10u;
    const uint32_t before = st.form.tracers;
    // (ER_STREAM_FORCE_BUSY: test knob -- the reading the mechanism is driven with instead of the measured one, whatever the launch's length;
    // the occupancy itself depends on clocks and may not be asserted on)
    // (a comma-separated list gives the k-th reading of the render its k-th value, the last one from then on)
    const char* forced = getenv("ER_STREAM_FORCE_BUSY");
    double busy = st.busy;
    if (forced) {
        const char* q = forced;
        for (uint32_t k = 0; k < st.readings; k++) { const char* c = strchr(q, ','); if (!c) break; q = c + 1; }
        busy = atof(q);
    }
    st.readings++;
    if (!forced && st.launch_ms < ER_STREAM_ADAPT_MIN_MS) {
        if (verbose) fprintf(stderr, "[er_stream] tracer lanes %.3f full in a launch of %.2f ms: too short to be a reading\n", st.busy, st.launch_ms);
        return;
    }
    if (busy < 0.85) {
        if (++st.low_streak >= 2u && st.form.tracers > lo) { st.form.tracers--; st.low_streak = 0; }
    } else {
        st.low_streak = 0;
        if (busy > 0.93 && st.up_budget > 0u && st.form.tracers < st.tracers_start) { st.form.tracers++; st.up_budget--; }
    }
    if (verbose) fprintf(stderr, "[er_stream] tracer lanes %.3f full%s at %u + %u waves -> %u + %u\n", busy, forced ? " (forced reading)" : "", before, st.form.waves - before, st.form.tracers, st.form.waves - st.form.tracers);
}

void stream_fill_info(const ErScene* s, ErStreamInfo* out) {
    const StreamHost& st = s->st;
    out->waves = st.form.waves; out->tracers = st.form.tracers;
    out->large_regions = st.large_deal_in_use() ? 1u : 0u;
    out->deal_pending = st.deal_pending ? 1u : 0u;
    out->launches = (uint32_t)st.launches;
    out->pixels_per_cu = (uint32_t)((size_t)s->dev.owned_tile_count * 64 / std::max<uint32_t>(1u, st.blocks));
    out->lanes_busy = st.busy; out->launch_ms = st.launch_ms; out->cost_spread = st.cost_spread;
    out->spec_started = st.spec[0]; out->spec_right = st.spec[1]; out->spec_wrong = st.spec[2];
    out->form = er_stream_launch_form(s->dev.max_bounces, s->tri_count, st.form.waves, st.form.spec, st.form.keep).form;      // (what er_launch_stream launches)
}
