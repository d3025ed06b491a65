// rxg_ops.cpp — the operations on a burst beside its classification (include/rxg.h): tx
// checksums, segment build with and without options, reset build, transmit planner,
// received-option parse, flow summary, flow trains, train payload, ACK plan.  Each entry point checks its
// arguments,
// fills its kernels' launch struct (rxg_kernels.h) and launches on the caller's stream; what
// they share -- rec_align, check_frame_src, grid_cap, SerialScratch -- is in rxg_ctx.h.
#include <cstring>

#include "rxg_ctx.h"

using namespace rxg;

extern "C" int rxg_tx_cksum_dev(rxg_ctx *c, const rxg_dev_tx_batch *b, void *stream)
{
    if (!c || !b) return fail(-EINVAL, "rxg_tx_cksum_dev: NULL argument");
    if (b->n && (!b->frames || !b->off64 || !b->len))
        return fail(-EINVAL, "rxg_tx_cksum_dev: NULL device pointer");
    if (b->n && (((uintptr_t)b->frames & 15u) || ((uintptr_t)b->off64 & 3u) || ((uintptr_t)b->len & 1u)))
        return fail(-EINVAL, "rxg_tx_cksum_dev: frames need 16-byte, off64 4-byte, len 2-byte alignment");
    int rc = set_device(c);
    if (rc) return rc;
    LaunchBurst one{b->off64, b->len, b->n, nullptr, 0u};
    LaunchRx L;
    std::memset(&L, 0, sizeof L);
    L.frames = (const uint8_t *)b->frames;
    L.bursts = &one;
    L.nbursts = 1;
    L.mode = 0;
    L.counters = nullptr;
    L.max_blocks = grid_for(c, 0);
    HIP_OK(launch_rx(L, pick(c, stream)));
    return 0;
}

static_assert(sizeof(rxg_tx_flow) == 32 && sizeof(rxg_tx_seg) == 32 && sizeof(rxg_dev_tx_build) == 80,
              "transmit segment build layouts");

// rxg_tx_build_dev and rxg_tx_build_opt_dev (`opt`: its block table): one argument check, one launch
static int tx_build_call(const char *who, rxg_ctx *c, const rxg_dev_tx_build *b, const rxg_dev_tx_build_opt *opt,
                         void *stream)
{
    if (!c || !b) return fail(-EINVAL, "%s: NULL argument", who);
    if (b->n == 0) return 0;
    if (!b->payload || !b->flows || !b->segs || !b->frames || !b->len)
        return fail(-EINVAL, "%s: NULL device pointer", who);
    if (((uintptr_t)b->payload & 15u) || ((uintptr_t)b->frames & 63u) || ((uintptr_t)b->segs & 7u) ||
        ((uintptr_t)b->flows & 7u) || ((uintptr_t)b->off64 & 3u) || ((uintptr_t)b->len & 1u) ||
        ((uintptr_t)b->stats & 7u))
        return fail(-EINVAL, "%s: payload needs 16-byte, frames 64-byte, segs, flows and stats "
                             "8-byte, off64 4-byte, len 2-byte alignment", who);
    int rc = check_frame_src(who, b->off64, b->slot0, b->stride64, b->n);
    if (rc) return rc;
    if (opt) {
        if ((uintptr_t)opt->opts & 15u) return fail(-EINVAL, "%s: opts needs 16-byte alignment", who);
        if (!opt->opts && opt->nopts) return fail(-EINVAL, "%s: NULL opts with nopts %u", who, opt->nopts);
    }
    if ((rc = set_device(c))) return rc;
    LaunchTxBuild L;
    L.payload = (const uint8_t *)b->payload;
    L.payload_bytes = b->payload_bytes;
    L.flows = b->flows;
    L.nflows = b->nflows;
    L.n = b->n;
    L.segs = b->segs;
    L.frames = (uint8_t *)b->frames;
    L.off64 = b->off64;
    L.slot0 = b->slot0;
    L.stride64 = b->stride64;
    L.len = b->len;
    L.stats = (unsigned long long *)b->stats;
    L.max_blocks = grid_cap(c, c->op_grid[opt ? kGridTxBuildOpt : kGridTxBuild]);
    L.with_opts = opt != nullptr;
    L.opts = opt ? opt->opts : nullptr;
    L.nopts = opt ? opt->nopts : 0u;
    HIP_OK(launch_tx_build(L, pick(c, stream)));
    return 0;
}

extern "C" int rxg_tx_build_dev(rxg_ctx *c, const rxg_dev_tx_build *b, void *stream)
{
    return tx_build_call("rxg_tx_build_dev", c, b, nullptr, stream);
}

static_assert(sizeof(rxg_tx_opt) == 48 && sizeof(rxg_dev_tx_build_opt) == 96, "option build layouts");

extern "C" int rxg_tx_build_opt_dev(rxg_ctx *c, const rxg_dev_tx_build_opt *b, void *stream)
{
    return tx_build_call("rxg_tx_build_opt_dev", c, b ? &b->b : nullptr, b, stream);
}

static_assert(sizeof(rxg_dev_tx_reset) == 88, "reset build layout");

extern "C" int rxg_tx_reset_dev(rxg_ctx *c, const rxg_dev_tx_reset *b, void *stream)
{
    if (!c || !b) return fail(-EINVAL, "rxg_tx_reset_dev: NULL argument");
    if (!b->frames || !b->len || !b->recs || !b->out || !b->idx || !b->count)
        return fail(-EINVAL, "rxg_tx_reset_dev: NULL device pointer");
    if (!rec_kind_ok(b->rec_kind)) return fail(-EINVAL, "rxg_tx_reset_dev: rec_kind %u", b->rec_kind);
    if (((uintptr_t)b->frames & 15u) || ((uintptr_t)b->out & 63u) || ((uintptr_t)b->idx & 3u) ||
        ((uintptr_t)b->off64 & 3u) || ((uintptr_t)b->len & 1u) || ((uintptr_t)b->count & 7u) ||
        ((uintptr_t)b->recs & (rec_align(b->rec_kind) - 1u)))
        return fail(-EINVAL, "rxg_tx_reset_dev: frames need 16-byte, out 64-byte, idx and off64 4-byte, len 2-byte, "
                             "count 8-byte, recs %u-byte alignment", (unsigned)rec_align(b->rec_kind));
    int rc = check_frame_src("rxg_tx_reset_dev", b->off64, b->slot0, b->stride64, b->n);
    if (rc) return rc;
    if ((rc = set_device(c))) return rc;
    hipStream_t st = pick(c, stream);
    LaunchTxReset L;
    L.src = FrameSrc{(const uint8_t *)b->frames, b->off64, b->len, b->slot0, b->stride64};
    L.n = b->n;
    L.rec_kind = b->rec_kind;
    L.recs = (const uint8_t *)b->recs;
    L.out = (uint8_t *)b->out;
    L.idx = b->idx;
    L.cap = b->cap;
    L.count = (unsigned long long *)b->count;
    L.counts = nullptr;
    L.ip_id0 = b->ip_id0;
    std::memcpy(L.src_mac, b->src_mac, 6);
    L.max_blocks = grid_cap(c, c->op_grid[kGridTxReset]);
    if (b->n) {
        DevBuf &counts = c->rst.buf[0];
        if ((rc = c->rst.grow(counts, tx_reset_count_bytes(b->n), false, st))) return rc;
        if ((rc = c->rst.begin(st))) return rc;
        L.counts = (uint32_t *)counts.p;
    }
    return c->rst.end(st, launch_tx_reset(L, st));
}

static_assert(sizeof(rxg_tx_send) == 40 && sizeof(rxg_dev_tx_plan) == 80, "device planner layouts");

extern "C" int rxg_tx_plan_dev(rxg_ctx *c, const rxg_dev_tx_plan *b, void *stream)
{
    if (!c || !b) return fail(-EINVAL, "rxg_tx_plan_dev: NULL argument");
    if (!b->sends || !b->first || !b->count || (!b->segs && b->cap))
        return fail(-EINVAL, "rxg_tx_plan_dev: NULL device pointer");
    if (((uintptr_t)b->sends & 7u) || ((uintptr_t)b->segs & 7u) || ((uintptr_t)b->first & 7u) ||
        ((uintptr_t)b->count & 7u) || ((uintptr_t)b->opts & 15u) || ((uintptr_t)b->next_seq & 3u) ||
        ((uintptr_t)b->send_opt & 3u))
        return fail(-EINVAL, "rxg_tx_plan_dev: sends, segs, first and count need 8-byte, opts 16-byte, next_seq and "
                             "send_opt 4-byte alignment");
    if (b->mss == 0 || b->mss > RXG_TX_MAX_DATA) return fail(-EINVAL, "rxg_tx_plan_dev: mss %u", b->mss);
    if (!b->opts && b->nopts) return fail(-EINVAL, "rxg_tx_plan_dev: NULL opts with nopts %u", b->nopts);
    int rc = set_device(c);
    if (rc) return rc;
    hipStream_t st = pick(c, stream);
    LaunchTxPlan L;
    L.sends = b->sends;
    L.nsends = b->nsends;
    L.mss = b->mss;
    L.send_opt = b->send_opt;
    L.opts = b->opts;
    L.nopts = b->nopts;
    L.segs = b->segs;
    L.cap = b->cap;
    L.first = (unsigned long long *)b->first;
    L.next_seq = b->next_seq;
    L.count = (unsigned long long *)b->count;
    L.tiles = nullptr;
    L.max_blocks = grid_cap(c, c->op_grid[kGridTxPlan]);
    if (b->nsends) {
        DevBuf &tiles = c->txp.buf[0];
        if ((rc = c->txp.grow(tiles, tx_plan_tile_bytes(b->nsends), false, st))) return rc;
        if ((rc = c->txp.begin(st))) return rc;
        L.tiles = tiles.p;
    }
    return c->txp.end(st, launch_tx_plan(L, st));
}

static_assert(sizeof(rxg_rx_opt) == 16 && sizeof(rxg_dev_rx_opts) == 56, "received-option layouts");

extern "C" int rxg_rx_opts_dev(rxg_ctx *c, const rxg_dev_rx_opts *b, void *stream)
{
    if (!c || !b) return fail(-EINVAL, "rxg_rx_opts_dev: NULL argument");
    if (!b->frames || !b->len || !b->recs || !b->out) return fail(-EINVAL, "rxg_rx_opts_dev: NULL device pointer");
    if (!rec_kind_ok(b->rec_kind)) return fail(-EINVAL, "rxg_rx_opts_dev: rec_kind %u", b->rec_kind);
    if (((uintptr_t)b->frames & 15u) || ((uintptr_t)b->out & 15u) || ((uintptr_t)b->off64 & 3u) ||
        ((uintptr_t)b->len & 1u) || ((uintptr_t)b->recs & (rec_align(b->rec_kind) - 1u)))
        return fail(-EINVAL, "rxg_rx_opts_dev: frames and out need 16-byte, off64 4-byte, len 2-byte, recs %u-byte "
                             "alignment", (unsigned)rec_align(b->rec_kind));
    int rc = check_frame_src("rxg_rx_opts_dev", b->off64, b->slot0, b->stride64, b->n);
    if (rc) return rc;
    if (!b->n) return 0;
    if ((rc = set_device(c))) return rc;
    LaunchRxOpts L;
    L.src = FrameSrc{(const uint8_t *)b->frames, b->off64, b->len, b->slot0, b->stride64};
    L.n = b->n;
    L.rec_kind = b->rec_kind;
    L.recs = (const uint8_t *)b->recs;
    L.out = (uint8_t *)b->out;
    L.max_blocks = grid_cap(c, c->op_grid[kGridRxOpts]);
    HIP_OK(launch_rx_opts(L, pick(c, stream)));
    return 0;
}

static_assert(sizeof(rxg_flow_sum) == 40 && sizeof(rxg_dev_flow_sums) == 80, "flow summary layouts");

extern "C" int rxg_flow_sums_dev(rxg_ctx *c, const rxg_dev_flow_sums *b, void *stream)
{
    if (!c || !b) return fail(-EINVAL, "rxg_flow_sums_dev: NULL argument");
    if (!rec_kind_ok(b->rec_kind)) return fail(-EINVAL, "rxg_flow_sums_dev: rec_kind %u", b->rec_kind);
    const bool reads_frames = b->rec_kind != RXG_REC48;
    if (!b->recs || !b->count || (!b->out && b->cap) || (reads_frames && (!b->frames || !b->len)))
        return fail(-EINVAL, "rxg_flow_sums_dev: NULL device pointer");
    if (b->ntcb == 0 || b->ntcb > RXG_FS_MAX_NTCB) return fail(-EINVAL, "rxg_flow_sums_dev: ntcb %u", b->ntcb);
    if (b->flags & ~RXG_FS_TCP_OK_ONLY) return fail(-EINVAL, "rxg_flow_sums_dev: unknown flags 0x%x", b->flags);
    if (((uintptr_t)b->frames & 15u) || ((uintptr_t)b->out & 7u) || ((uintptr_t)b->count & 7u) ||
        ((uintptr_t)b->off64 & 3u) || ((uintptr_t)b->len & 1u) || ((uintptr_t)b->recs & (rec_align(b->rec_kind) - 1u)))
        return fail(-EINVAL, "rxg_flow_sums_dev: frames need 16-byte, out and count 8-byte, off64 4-byte, len 2-byte, "
                             "recs %u-byte alignment", (unsigned)rec_align(b->rec_kind));
    int rc = reads_frames ? check_frame_src("rxg_flow_sums_dev", b->off64, b->slot0, b->stride64, b->n) : 0;
    if (rc) return rc;
    if ((rc = set_device(c))) return rc;
    hipStream_t st = pick(c, stream);
    LaunchFlowSum L;
    L.src = FrameSrc{reads_frames ? (const uint8_t *)b->frames : nullptr, b->off64, b->len, b->slot0, b->stride64};
    L.n = b->n;
    L.rec_kind = b->rec_kind;
    L.recs = (const uint8_t *)b->recs;
    L.ntcb = b->ntcb;
    L.flags = b->flags;
    L.out = b->out;
    L.cap = b->cap;
    L.count = (unsigned long long *)b->count;
    L.acc = nullptr;
    L.bits = nullptr;
    L.tiles = nullptr;
    L.max_blocks = c->max_blocks;
    // (the accumulation's own grid; launch_flow_sum applies max_blocks on top of it)
    L.acc_blocks = c->op_grid[kGridFlowSum] ? c->op_grid[kGridFlowSum] : 1024u;
    if (b->n) {
        DevBuf &acc = c->fs.buf[rxg_ctx::kFsAcc], &bits = c->fs.buf[rxg_ctx::kFsBits],
               &tiles = c->fs.buf[rxg_ctx::kFsTiles];
        if ((rc = c->fs.grow(acc, flow_sum_bytes(b->ntcb), true, st))) return rc;
        if ((rc = c->fs.grow(bits, flow_sum_bits_bytes(b->ntcb), true, st))) return rc;
        if ((rc = c->fs.grow(tiles, flow_sum_tile_bytes(b->ntcb), false, st))) return rc;
        if ((rc = c->fs.begin(st))) return rc;
        if (c->fs_dirty) {
            HIP_OK(hipMemsetAsync(acc.p, 0, acc.bytes, st));
            HIP_OK(hipMemsetAsync(bits.p, 0, bits.bytes, st));
            c->fs_dirty = false;
        }
        L.acc = (FlowSumAcc *)acc.p;
        L.bits = (uint32_t *)bits.p;
        L.tiles = (uint32_t *)tiles.p;
    }
    const hipError_t e = launch_flow_sum(L, st);
    if (b->n && e != hipSuccess) c->fs_dirty = true;
    return c->fs.end(st, e);
}

static_assert(sizeof(rxg_flow_train) == 32 && sizeof(rxg_dev_flow_trains) == 104, "flow train layouts");

extern "C" int rxg_flow_trains_dev(rxg_ctx *c, const rxg_dev_flow_trains *b, void *stream)
{
    if (!c || !b) return fail(-EINVAL, "rxg_flow_trains_dev: NULL argument");
    if (!rec_kind_ok(b->rec_kind)) return fail(-EINVAL, "rxg_flow_trains_dev: rec_kind %u", b->rec_kind);
    const bool reads_frames = b->rec_kind != RXG_REC48;
    if (!b->recs || !b->count || (!b->order && b->cap_seg) || (!b->trains && b->cap_trains) ||
        (reads_frames && (!b->frames || !b->len)))
        return fail(-EINVAL, "rxg_flow_trains_dev: NULL device pointer");
    if (b->ntcb == 0 || b->ntcb > RXG_FS_MAX_NTCB) return fail(-EINVAL, "rxg_flow_trains_dev: ntcb %u", b->ntcb);
    if (b->flags & ~RXG_FT_TCP_OK_ONLY) return fail(-EINVAL, "rxg_flow_trains_dev: unknown flags 0x%x", b->flags);
    if (((uintptr_t)b->frames & 15u) || ((uintptr_t)b->trains & 7u) || ((uintptr_t)b->count & 7u) ||
        ((uintptr_t)b->cur_seq & 3u) || ((uintptr_t)b->order & 3u) || ((uintptr_t)b->off64 & 3u) ||
        ((uintptr_t)b->len & 1u) || ((uintptr_t)b->recs & (rec_align(b->rec_kind) - 1u)))
        return fail(-EINVAL, "rxg_flow_trains_dev: frames need 16-byte, trains and count 8-byte, cur_seq, order and "
                             "off64 4-byte, len 2-byte, recs %u-byte alignment", (unsigned)rec_align(b->rec_kind));
    int rc = reads_frames ? check_frame_src("rxg_flow_trains_dev", b->off64, b->slot0, b->stride64, b->n) : 0;
    if (rc) return rc;
    if ((rc = set_device(c))) return rc;
    hipStream_t st = pick(c, stream);
    LaunchFlowTrain L;
    L.src = FrameSrc{reads_frames ? (const uint8_t *)b->frames : nullptr, b->off64, b->len, b->slot0, b->stride64};
    L.n = b->n;
    L.rec_kind = b->rec_kind;
    L.recs = (const uint8_t *)b->recs;
    L.ntcb = b->ntcb;
    L.flags = b->flags;
    L.cur_seq = b->cur_seq;
    L.order = b->order;
    L.cap_seg = b->cap_seg;
    L.trains = b->trains;
    L.cap_trains = b->cap_trains;
    L.count = (unsigned long long *)b->count;
    L.pairs = nullptr;
    L.meta = nullptr;
    L.counts = nullptr;
    L.max_blocks = grid_cap(c, c->op_grid[kGridFlowTrain]);
    if (b->n) {
        DevBuf &pairs = c->ft.buf[rxg_ctx::kFtPairs], &meta = c->ft.buf[rxg_ctx::kFtMeta],
               &counts = c->ft.buf[rxg_ctx::kFtCounts];
        if ((rc = c->ft.grow(pairs, flow_train_pair_bytes(b->n), false, st))) return rc;
        if ((rc = c->ft.grow(meta, flow_train_meta_bytes(b->n), false, st))) return rc;
        if ((rc = c->ft.grow(counts, flow_train_count_bytes(b->n), false, st))) return rc;
        if ((rc = c->ft.begin(st))) return rc;
        L.pairs = pairs.p;
        L.meta = meta.p;
        L.counts = (uint32_t *)counts.p;
    }
    return c->ft.end(st, launch_flow_train(L, st));
}

static_assert(sizeof(rxg_dev_train_payload) == 136, "train payload layout");

extern "C" int rxg_train_payload_dev(rxg_ctx *c, const rxg_dev_train_payload *b, void *stream)
{
    if (!c || !b) return fail(-EINVAL, "rxg_train_payload_dev: NULL argument");
    if (!rec_kind_ok(b->rec_kind)) return fail(-EINVAL, "rxg_train_payload_dev: rec_kind %u", b->rec_kind);
    if (!b->frames || !b->len || !b->recs || !b->count || !b->arena_used || (!b->order && b->cap_seg) ||
        (!b->trains && b->cap_trains) || (!b->arena && b->arena_cap))
        return fail(-EINVAL, "rxg_train_payload_dev: NULL device pointer");
    if (b->flags & ~RXG_TP_HEAD_ONLY) return fail(-EINVAL, "rxg_train_payload_dev: unknown flags 0x%x", b->flags);
    if (((uintptr_t)b->frames & 15u) || ((uintptr_t)b->arena & 15u) || ((uintptr_t)b->msgs & 7u) ||
        ((uintptr_t)b->tmsgs & 7u) || ((uintptr_t)b->trains & 7u) || ((uintptr_t)b->count & 7u) ||
        ((uintptr_t)b->arena_used & 7u) || ((uintptr_t)b->order & 3u) || ((uintptr_t)b->off64 & 3u) ||
        ((uintptr_t)b->len & 1u) || ((uintptr_t)b->recs & (rec_align(b->rec_kind) - 1u)))
        return fail(-EINVAL, "rxg_train_payload_dev: frames and arena need 16-byte, msgs, tmsgs, trains, count and "
                             "arena_used 8-byte, order and off64 4-byte, len 2-byte, recs %u-byte alignment",
                    (unsigned)rec_align(b->rec_kind));
    int rc = check_frame_src("rxg_train_payload_dev", b->off64, b->slot0, b->stride64, b->n);
    if (rc) return rc;
    if ((rc = set_device(c))) return rc;
    hipStream_t st = pick(c, stream);
    LaunchTrainPay L;
    L.src = FrameSrc{(const uint8_t *)b->frames, b->off64, b->len, b->slot0, b->stride64};
    L.n = b->n;
    L.rec_kind = b->rec_kind;
    L.recs = (const uint8_t *)b->recs;
    L.order = b->order;
    L.cap_seg = b->cap_seg;
    L.trains = b->trains;
    L.cap_trains = b->cap_trains;
    L.count = (const unsigned long long *)b->count;
    L.flags = b->flags;
    L.arena = (uint8_t *)b->arena;
    L.arena_cap = b->arena ? b->arena_cap : 0;
    L.msgs = b->msgs;
    L.tmsgs = b->tmsgs;
    L.used = (unsigned long long *)b->arena_used;
    L.scratch = nullptr;
    L.max_blocks = grid_cap(c, c->op_grid[kGridTrainPay]);
    // one gather or train payload in flight per context (rxg_payload_gather_dev's rule): the
    // messages rxg_payload_take reads are the last such call's
    if (b->msgs && c->pm.ev) HIP_OK(hipStreamWaitEvent(st, c->pm.ev, 0));
    if (b->n) {
        DevBuf &scratch = c->tp.buf[0];
        if ((rc = c->tp.grow(scratch, train_pay_scratch_bytes(b->n, b->cap_trains), false, st))) return rc;
        if ((rc = c->tp.begin(st))) return rc;
        L.scratch = scratch.p;
    }
    if ((rc = c->tp.end(st, launch_train_pay(L, st)))) return rc;
    return b->msgs ? pm_handoff(c, st, b->msgs, b->arena_used, b->n) : 0;
}

static_assert(sizeof(rxg_ack_state) == 16 && sizeof(rxg_ack) == 16 && sizeof(rxg_dev_ack_plan) == 128,
              "ACK plan layouts");

extern "C" int rxg_ack_plan_dev(rxg_ctx *c, const rxg_dev_ack_plan *b, void *stream)
{
    if (!c || !b) return fail(-EINVAL, "rxg_ack_plan_dev: NULL argument");
    if (!b->train_count || !b->state || !b->count || (!b->order && b->cap_seg) || (!b->trains && b->cap_trains) ||
        ((!b->segs || !b->acks) && b->cap))
        return fail(-EINVAL, "rxg_ack_plan_dev: NULL device pointer");
    if (b->ntcb == 0 || b->ntcb > RXG_FS_MAX_NTCB) return fail(-EINVAL, "rxg_ack_plan_dev: ntcb %u", b->ntcb);
    if (b->flags) return fail(-EINVAL, "rxg_ack_plan_dev: unknown flags 0x%x", b->flags);
    if (b->opt_plain > b->opt_base || b->opt_base > b->opt_cap)
        return fail(-EINVAL, "rxg_ack_plan_dev: opt_plain %u, opt_base %u, opt_cap %u", b->opt_plain, b->opt_base,
                    b->opt_cap);
    if (((uintptr_t)b->state & 15u) || ((uintptr_t)b->rxopts & 15u) || ((uintptr_t)b->opts & 15u) ||
        ((uintptr_t)b->segs & 15u) || ((uintptr_t)b->acks & 15u) || ((uintptr_t)b->trains & 7u) ||
        ((uintptr_t)b->train_count & 7u) || ((uintptr_t)b->count & 7u) || ((uintptr_t)b->order & 3u))
        return fail(-EINVAL, "rxg_ack_plan_dev: state, rxopts, opts, segs and acks need 16-byte, trains, train_count "
                             "and count 8-byte, order 4-byte alignment");
    int rc = set_device(c);
    if (rc) return rc;
    hipStream_t st = pick(c, stream);
    LaunchAckPlan L;
    L.order = b->order;
    L.cap_seg = b->order ? b->cap_seg : 0;
    L.trains = b->trains;
    L.cap_trains = b->trains ? b->cap_trains : 0;
    L.train_count = (const unsigned long long *)b->train_count;
    L.n = b->n;
    L.ntcb = b->ntcb;
    L.rxopts = b->rxopts;
    L.state = b->state;
    L.tsval_now = b->tsval_now;
    L.ip_id0 = b->ip_id0;
    L.opt_plain = b->opt_plain;
    L.opt_base = b->opt_base;
    L.opt_cap = b->opt_cap;
    L.opts = b->opts;
    L.segs = b->segs;
    L.acks = b->acks;
    L.cap = b->cap;
    L.count = (unsigned long long *)b->count;
    L.scratch = nullptr;
    L.max_blocks = grid_cap(c, c->op_grid[kGridAckPlan]);
    const size_t bytes = ack_plan_scratch_bytes(b->n, L.cap_trains);
    if (bytes) {
        DevBuf &scratch = c->ak.buf[0];
        if ((rc = c->ak.grow(scratch, bytes, false, st))) return rc;
        if ((rc = c->ak.begin(st))) return rc;
        L.scratch = scratch.p;
    }
    return c->ak.end(st, launch_ack_plan(L, st));
}
