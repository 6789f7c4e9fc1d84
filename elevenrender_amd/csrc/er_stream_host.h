// er_stream_host.h -- host side of the streaming schedule (er_stream_host.cpp): its state in a scene (ErScene::st) and everything that
// touches it -- the deal of tiles, the choice of the kernel's form, set-up at er_render_begin, the re-deal of an adaptive render, the
// launches, the status read-back and the adaptation between calls.
#pragma once
#include <stdint.h>

#include <vector>

#include "er_devbuf.h"
#include "er_stream.h"

struct ErScene;
struct ErStreamInfo;

// The streaming kernel's form for a share: waves per workgroup, how many of them trace, and whether the split follows the lanes'
// occupancy (adapt), pixels that are behind keep their slots (keep), speculative samples are started (spec).
struct StreamForm {
    uint32_t waves = 16, tracers = 0;
    bool adapt = false, keep = false, spec = false;
};
// A pure function of its arguments and the A/B knobs of the environment (read per call): share in tiles, workgroups, whether the
// slots carry a light query (point lights or emitters), the scene's triangles, the render's flags (ER_FLAG_COUNTERS).
StreamForm stream_choose_form(size_t tiles, uint32_t blocks, bool light_query, uint32_t tri_count, uint32_t flags);
// which deal of tiles the schedule uses for a share of `owned_tiles` tiles on `blocks` workgroups
bool stream_xcd_aware(size_t owned_tiles, uint32_t blocks);

// a deal of tiles to workgroups (er_stream_deal_tiles) and the largest number of tiles any workgroup got
struct StreamDeal {
    std::vector<uint32_t> tiles;
    uint32_t most = 0;
};
// the deal er_render_begin chooses the schedule on and the streaming schedule then starts with: the owned share, default edge
StreamDeal stream_deal_owned(const std::vector<uint32_t>& owned, uint32_t tiles_x, uint32_t cus);

struct StreamHost {
    uint32_t blocks = 0;                  // workgroups: one per CU
    uint32_t ring_cap = 0;                // cells of a workgroup's pixel ring
    bool lights = false;                  // slot records carry a light query's line
    StreamForm form;                      // stream_choose_form's for the share in use, EXCEPT form.tracers, which then moves with the readings (stream_adapt)
    uint32_t tracers_start = 0;           //   the split the share began with
    uint32_t low_streak = 0;              //   consecutive low readings
    uint32_t up_budget = 1;               //   steps back up left
    uint32_t readings = 0;                //   readings of this render (ER_STREAM_FORCE_BUSY indexes them)
    uint32_t* ctl = nullptr;              // ER_STREAM_CTL_LEAD + er_stream_ctl_words(blocks) control words (a view into ErScene::d_wf1); the kernel's `status` is ...
    uint32_t* status() const { return ctl + ER_STREAM_CTL_LEAD; }
    double busy = 0.0;                    // tracer lanes that held a ray, last completed call
    double launch_ms = 0.0;               // device time of that call's launch (start stamp to the last XCD's end stamp)
    uint64_t launch_start = 0, launch_end = 0;   // that launch's start stamp and the last XCD's end stamp (100 MHz ticks; 0: none)
    std::vector<uint64_t> wg_end;         // ... and every workgroup's end stamp (0: the workgroup ran no wave); printed and logged, nothing is decided on them
    double xcd_spread = 0.0;              // (latest - earliest XCD) / launch duration of the last completed call; < 0: not measured
    double cost_spread = -1.0;            // (max - min) / mean of the XCDs' counted work under the large deal; < 0: not decided yet
    uint64_t spec[3] = {0, 0, 0};         // speculative samples started / right / wrong, summed over the render's completed launches
    uint64_t spec_seen = 0;               //   ... the launch up to which they have been added
    uint64_t launches = 0, adapted = 0;   // launches enqueued / the launch whose measurements stream_adapt has already used
    bool probe_launch = false;            // the launch just completed was a render's first sample, run alone to decide the deal
    // d_deal holds the deal the render began with, while a render has it the deal of large screen regions behind it, and behind both
    // room for the one of the two that was taken, levelled by counted cost (blocks * ring_cap / 64 entries: the rings do not grow)
    erh::DevBuf<uint32_t> d_deal, d_ticket;      // d_ticket: the workgroups' pixel rings
    uint32_t deal_off = 0, deal_n = 0;          // the deal in use inside d_deal (entries)
    uint32_t deal_alt_off = 0, deal_alt_n = 0;  // the deal of large screen regions beside it (0 entries: none)
    uint32_t deal_base_off = 0;                 // the deal of the two that was taken (the one in use unless it has been levelled)
    uint32_t deal_lvl_off = 0, deal_lvl_cap = 0;   // where the levelled deal goes in d_deal and how many entries fit (0: none)
    bool deal_levelled = false;                 // the deal in use is deal_base levelled by counted cost
    bool counting = false;                      // the kernel is adding path lengths to d_tile_cost: from er_render_begin until the first CALL has completed
    std::vector<uint32_t> deal_base;            // host copy of the deal that was taken, while counting (what is levelled)
    std::vector<uint32_t> deal_host;            // host copy of the deal in use (er_debug_stream_balance)
    std::vector<uint32_t> cost_host;            // the tile costs last read (er_debug_stream_balance)
    bool deal_pending = false;                  // the first completed launch decides between the two (stream_adapt), from ...
    erh::DevBuf<uint32_t> d_tile_cost;          // ... DevScene::tile_cost: per tile of the frame, the summed path lengths of its finished samples
    std::vector<uint32_t> deal_large;           // host copy of the large deal until then (which XCD gets which tile under it)
    erh::DevBuf<uint32_t> d_px_draws;           // DevScene::px_draws

    bool large_deal_in_use() const { return deal_alt_n != 0u && deal_base_off == deal_alt_off; }      // (pending: the default deal, at offset 0, is in use)
    void release() {
        d_deal.release(); d_ticket.release(); d_tile_cost.release(); d_px_draws.release();
        ctl = nullptr;
    }
};

// All of these are called with the scene's mutex held.
// er_render_begin, ER_FLAG_STREAM: buffers, both deals, pixel rings.  `deal` is stream_deal_owned(owned, ...) (it is changed).
int stream_begin(ErScene* s, const std::vector<uint32_t>& owned, StreamDeal& deal, uint32_t cus, bool light_query);
// an adaptive render's new active share (ErScene::ad_active): its deal and form, within the buffers stream_begin made
int stream_redeal(ErScene* s);
// n more samples to every tile of the deal
int stream_enqueue(ErScene* s, uint32_t n);
// after a completed launch (the stream is idle): the deal decision and the tracer / shader split
void stream_adapt(ErScene* s);
void stream_fill_info(const ErScene* s, ErStreamInfo* out);
// per workgroup of the deal in use: tiles, counted cost (the tile costs last read), end stamp minus launch start of the last completed launch
void stream_balance(const ErScene* s, std::vector<uint32_t>& wg_tiles, std::vector<uint64_t>& wg_cost, std::vector<uint64_t>& wg_ticks);
