// k_state.hip -- snapshots of one sequence's tracker state (lvt_amd_snapshot_*, include/lvt_amd_ext.h): the blob and the two kernels that fill and empty it.
//
// THE BLOB: one contiguous device allocation per snapshot; its exported form is the same bytes.
//   SnapHeader | Ctl | map pos | map desc | map counter | map age | staged pos | staged desc | staged counter
// Every section starts on a 16-byte boundary, padding bytes are zero, only the first map_n / staged_n points of the LIVE ping-pong copy are stored, in
// storage order (MapSoA::match_idx is per-frame scratch and stays out).  The Ctl section is the sequence's record with every word that belongs to a LAUNCH
// CHAIN, not to the tracker, zeroed (ChainWords below + Ctl::dbg): two takes of one state hold the same bytes whatever route the frames took, and a snapshot
// taken right after an apply holds the bytes that were applied.  The header is written by the host (the checksum at export).
//
// THE KERNELS: k_state_pack gathers up to STATE_PACK sequences into their blobs in one launch, k_state_unpack scatters blobs back into sequences; the
// per-sequence descriptors travel BY VALUE (as RectTable / GrayTable do), blockIdx.y = sequence, the grid's x extent follows the largest sequence and a
// smaller one's surplus workgroups leave at the top.  Every array moves as 16-byte loads and stores between the first 16-byte boundary of its source and its
// last whole vector, with single elements on either side (k_stage_copy's rule): no load or store reaches outside its section.  Source and destination of a
// section are aligned alike (device allocations and section offsets are multiples of 16; the host checks it before it launches).
#pragma once
#include "lvt_dev.h"
#include "../../include/lvt_amd_ext.h"
#include <cstddef>
#include <cstring>

namespace lvt {

constexpr uint64_t SNAP_MAGIC = 0x31504E535F54564Cull;  // "LVT_SNP1"
constexpr int SNAP_VERSION = 1;
enum : int { SEC_CTL = 0, SEC_MAP_POS, SEC_MAP_DESC, SEC_MAP_COUNTER, SEC_MAP_AGE, SEC_ST_POS, SEC_ST_DESC, SEC_ST_COUNTER, SNAP_SECTIONS };

struct SnapHeader {
    uint64_t magic;
    int version, header_bytes, ctl_bytes;   // sizeof(SnapHeader), sizeof(Ctl) of the library that took it
    int nf_max, map_max, staged_max;        // the capacities it was built with
    int sensor;
    int map_n, staged_n;                    // points stored
    int map_cur, staged_cur;                // the ping-pong copies they were live in (an apply fills the same ones)
    int reserved0;
    lvt_amd_params prm;                     // the sequence's parameters as its creator handed them in
    int off[SNAP_SECTIONS];                 // byte offset of every section from the start of the blob
    int reserved1;
    long long total;                        // bytes of the whole blob
    uint64_t checksum;                      // of everything behind the header (snap_checksum); written at export, verified at import / describe
};
static_assert(sizeof(lvt_amd_params) == 100 && sizeof(SnapHeader) == 208 && sizeof(SnapHeader) % 16 == 0, "the header has no implicit padding and ends on a 16-byte boundary");

// bytes of the point sections per element: pos 3 doubles, desc 4 x 64 bits, counter / age one int
__host__ __device__ constexpr long long snap_pad16(long long b) { return (b + 15) & ~15ll; }
// section offsets of a blob with these point counts; returns its size
inline long long snap_layout(int map_n, int staged_n, int off[SNAP_SECTIONS]) {
    const long long bytes[SNAP_SECTIONS] = {(long long)sizeof(Ctl), 24ll * map_n, 32ll * map_n, 4ll * map_n, 4ll * map_n, 24ll * staged_n, 32ll * staged_n, 4ll * staged_n};
    long long o = sizeof(SnapHeader);
    for (int k = 0; k < SNAP_SECTIONS; k++) {
        off[k] = (int)o;
        o += snap_pad16(bytes[k]);
    }
    return o;
}
// 64-bit checksum of the payload (not cryptographic: it catches a damaged or cut file): FNV-1a over 64-bit words, the tail bytes one by one
inline uint64_t snap_checksum(const uint8_t *p, size_t n) {
    uint64_t h = 0xCBF29CE484222325ull;
    size_t i = 0;
    for (; i + 8 <= n; i += 8) {
        uint64_t w;
        __builtin_memcpy(&w, p + i, 8);
        h = (h ^ w) * 0x100000001B3ull;
        h ^= h >> 29;
    }
    for (; i < n; i++) h = (h ^ p[i]) * 0x100000001B3ull;
    return h;
}

// The words of Ctl that belong to a launch chain: sequence numbers handed between the three streams of ONE context, its gate counters and the skip flag.  They
// lie side by side in the record; a blob holds them as zero, an apply writes the target context's own (those of a just-reset record: reset_state).
struct ChainWords {
    seq_t pnp_seq, gate_ok, early_ran_seq, early_state, track_done_seq, late_gate_seq;
    int gate_timeouts, gate_fatal, skip;
};
struct ChainWordsArg {
    uint32_t w[15];
};
static_assert(sizeof(ChainWords) == 64 && offsetof(ChainWords, skip) == 56, "ChainWords mirrors Ctl::pnp_seq .. Ctl::skip");
static_assert(offsetof(Ctl, gate_ok) == offsetof(Ctl, pnp_seq) + 8 && offsetof(Ctl, early_ran_seq) == offsetof(Ctl, pnp_seq) + 16 &&
                  offsetof(Ctl, early_state) == offsetof(Ctl, pnp_seq) + 24 && offsetof(Ctl, track_done_seq) == offsetof(Ctl, pnp_seq) + 32 &&
                  offsetof(Ctl, late_gate_seq) == offsetof(Ctl, pnp_seq) + 40 && offsetof(Ctl, gate_timeouts) == offsetof(Ctl, pnp_seq) + 48 &&
                  offsetof(Ctl, gate_fatal) == offsetof(Ctl, pnp_seq) + 52 && offsetof(Ctl, skip) == offsetof(Ctl, pnp_seq) + 56,
              "the chain words of Ctl are contiguous, in ChainWords' order");
constexpr unsigned CTL_WORDS = sizeof(Ctl) / 4, CTL_WORDS_PADDED = (unsigned)(snap_pad16(sizeof(Ctl)) / 4);
constexpr unsigned CHAIN_W0 = offsetof(Ctl, pnp_seq) / 4, CHAIN_WN = 15, DBG_W0 = offsetof(Ctl, dbg) / 4, DBG_WN = sizeof(Ctl::dbg) / 4;
static_assert(sizeof(Ctl) % 4 == 0 && offsetof(Ctl, pnp_seq) % 4 == 0 && offsetof(Ctl, dbg) % 4 == 0, "Ctl is copied as 32-bit words");

inline ChainWords chain_of(const Ctl &z) {
    return ChainWords{z.pnp_seq, z.gate_ok, z.early_ran_seq, z.early_state, z.track_done_seq, z.late_gate_seq, z.gate_timeouts, z.gate_fatal, z.skip};
}
__host__ __device__ inline void set_chain(Ctl &k, const ChainWords &c) {  // (the record an apply leaves in the host ring; a relocalisation's commit on either side)
    k.pnp_seq = c.pnp_seq, k.gate_ok = c.gate_ok, k.early_ran_seq = c.early_ran_seq, k.early_state = c.early_state, k.track_done_seq = c.track_done_seq;
    k.late_gate_seq = c.late_gate_seq, k.gate_timeouts = c.gate_timeouts, k.gate_fatal = c.gate_fatal, k.skip = c.skip;
    for (unsigned i = 0; i < sizeof(k.dbg) / sizeof(k.dbg[0]); i++) k.dbg[i] = 0;
}
inline ChainWordsArg chain_arg(const ChainWords &c) {
    ChainWordsArg a;
    __builtin_memcpy(a.w, &c, sizeof(a.w));
    return a;
}

struct PointsRef {  // the arrays of a MapSoA that are state
    double *pos;
    uint64_t *desc;
    int *counter, *age;
};
struct StateSeq {
    Ctl *ctl;
    PointsRef map[2], staged[2];                    // both ping-pong copies (staged: age unused)
    int *map_cur, *map_n, *staged_cur, *staged_n;   // the sequence's device scalars
    uint8_t *blob;
    int off[SNAP_SECTIONS];
    int map_n_blob, staged_n_blob;      // points the blob has room for (pack) / holds (unpack)
    int map_cur_blob, staged_cur_blob;  // unpack: the copies to fill
};
// 16 descriptors of 224 bytes: the 14 array pointers alone take 112 of them, so 32 sequences cannot travel in one kernel-argument segment -- a batch of
// more than STATE_PACK sequences takes a second launch
constexpr int STATE_PACK = 16;
struct StateTable {
    StateSeq s[STATE_PACK];
};
static_assert(sizeof(StateTable) + sizeof(ChainWordsArg) + sizeof(int *) < 4096, "the state kernels' arguments must stay under 4096 bytes");

// what a workgroup of sequence-row y has to do, in 16-byte vectors of its longest section (desc: two per point) -- or in Ctl words, whichever is more
__host__ __device__ constexpr unsigned state_work(int map_n, int staged_n) {
    const unsigned pts = 2u * (unsigned)(map_n > staged_n ? map_n : staged_n);
    return pts > CTL_WORDS_PADDED ? pts : CTL_WORDS_PADDED;
}

// n elements src -> dst and `pad` zero elements behind them; src and dst are aligned alike
template <typename T>
__device__ __forceinline__ void copy_span(const T *src, T *dst, unsigned n, unsigned pad, unsigned t0, unsigned stride) {
    constexpr unsigned PER = 16 / sizeof(T);
    const unsigned head = min((unsigned)(((16 - ((uintptr_t)src & 15)) & 15) / sizeof(T)), n);
    const unsigned nv = (n - head) / PER, tail0 = head + nv * PER;
    for (unsigned v = t0; v < nv; v += stride) *reinterpret_cast<uint4 *>(dst + head + v * PER) = *reinterpret_cast<const uint4 *>(src + head + v * PER);
    if (t0 < head) dst[t0] = src[t0];
    if (t0 < n - tail0) dst[tail0 + t0] = src[tail0 + t0];
    if (t0 < pad) dst[n + t0] = T(0);
}
__device__ __forceinline__ unsigned pad_elems(unsigned n, unsigned elem_bytes) { return (unsigned)(snap_pad16((long long)n * elem_bytes) / elem_bytes) - n; }

// PACK: sequence -> blob (chain words and debug stamps zeroed, section padding zeroed); else blob -> sequence (chain words from cw, stamps zeroed, the
// sequence's scalars set to what was written)
template <bool PACK>
__device__ __forceinline__ void state_body(const StateSeq &D, const ChainWordsArg &cw, int *status) {
    int mcur, scur, mn, sn;
    if (PACK) {
        mcur = *D.map_cur & 1, scur = *D.staged_cur & 1;
        mn = min(max(*D.map_n, 0), D.map_n_blob), sn = min(max(*D.staged_n, 0), D.staged_n_blob);   // (never more than the blob has room for)
    } else {
        mcur = D.map_cur_blob & 1, scur = D.staged_cur_blob & 1;
        mn = min(max(D.map_n_blob, 0), MAP_MAX), sn = min(max(D.staged_n_blob, 0), STAGED_MAX);
    }
    if (blockIdx.x * 256u >= state_work(mn, sn)) return;   // a workgroup outside this sequence
    const unsigned t0 = blockIdx.x * 256u + threadIdx.x, stride = gridDim.x * 256u;
    {   // Ctl, word by word
        const uint32_t *src = PACK ? reinterpret_cast<const uint32_t *>(D.ctl) : reinterpret_cast<const uint32_t *>(D.blob + D.off[SEC_CTL]);
        uint32_t *dst = PACK ? reinterpret_cast<uint32_t *>(D.blob + D.off[SEC_CTL]) : reinterpret_cast<uint32_t *>(D.ctl);
        for (unsigned w = t0; w < (PACK ? CTL_WORDS_PADDED : CTL_WORDS); w += stride) {
            uint32_t v = 0;
            if (w - CHAIN_W0 < CHAIN_WN) v = PACK ? 0u : cw.w[w - CHAIN_W0];
            else if (w < CTL_WORDS && !(w - DBG_W0 < DBG_WN)) v = src[w];
            dst[w] = v;
        }
    }
    const PointsRef &M = D.map[mcur], &S = D.staged[scur];
    uint8_t *b = D.blob;
    const unsigned m = (unsigned)mn, s = (unsigned)sn;
    if (PACK) {
        copy_span(M.pos, reinterpret_cast<double *>(b + D.off[SEC_MAP_POS]), 3 * m, pad_elems(3 * m, 8), t0, stride);
        copy_span(M.desc, reinterpret_cast<uint64_t *>(b + D.off[SEC_MAP_DESC]), 4 * m, 0, t0, stride);
        copy_span(M.counter, reinterpret_cast<int *>(b + D.off[SEC_MAP_COUNTER]), m, pad_elems(m, 4), t0, stride);
        copy_span(M.age, reinterpret_cast<int *>(b + D.off[SEC_MAP_AGE]), m, pad_elems(m, 4), t0, stride);
        copy_span(S.pos, reinterpret_cast<double *>(b + D.off[SEC_ST_POS]), 3 * s, pad_elems(3 * s, 8), t0, stride);
        copy_span(S.desc, reinterpret_cast<uint64_t *>(b + D.off[SEC_ST_DESC]), 4 * s, 0, t0, stride);
        copy_span(S.counter, reinterpret_cast<int *>(b + D.off[SEC_ST_COUNTER]), s, pad_elems(s, 4), t0, stride);
        if (t0 == 0) status[0] = *D.map_cur, status[1] = *D.map_n, status[2] = *D.staged_cur, status[3] = *D.staged_n;   // what the host sized the blob for must be what is there
    } else {
        copy_span(reinterpret_cast<const double *>(b + D.off[SEC_MAP_POS]), M.pos, 3 * m, 0, t0, stride);
        copy_span(reinterpret_cast<const uint64_t *>(b + D.off[SEC_MAP_DESC]), M.desc, 4 * m, 0, t0, stride);
        copy_span(reinterpret_cast<const int *>(b + D.off[SEC_MAP_COUNTER]), M.counter, m, 0, t0, stride);
        copy_span(reinterpret_cast<const int *>(b + D.off[SEC_MAP_AGE]), M.age, m, 0, t0, stride);
        copy_span(reinterpret_cast<const double *>(b + D.off[SEC_ST_POS]), S.pos, 3 * s, 0, t0, stride);
        copy_span(reinterpret_cast<const uint64_t *>(b + D.off[SEC_ST_DESC]), S.desc, 4 * s, 0, t0, stride);
        copy_span(reinterpret_cast<const int *>(b + D.off[SEC_ST_COUNTER]), S.counter, s, 0, t0, stride);
        if (t0 == 0) *D.map_cur = mcur, *D.map_n = mn, *D.staged_cur = scur, *D.staged_n = sn;
    }
}

__global__ __launch_bounds__(256) void k_state_pack(StateTable tab, int *status) {
    const ChainWordsArg none{};
    state_body<true>(tab.s[blockIdx.y], none, status + 4 * blockIdx.y);   // (uniform index: the descriptor stays in scalar registers)
}
__global__ __launch_bounds__(256) void k_state_unpack(StateTable tab, ChainWordsArg cw) {
    state_body<false>(tab.s[blockIdx.y], cw, nullptr);
}

}  // namespace lvt
