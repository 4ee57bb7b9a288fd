// Node classification (include/graphem_hip.h "node classification" and "label propagation"; graphem-rapids_amd/classify.py):
// the exact k nearest labelled vertices of every query row with the vote of their classes, on the position snapshot of a
// gh_qual handle, and synchronous label propagation with clamped seeds over the centrality handle's CSR.
//
// The k-NN rule is the header's: the distance is qual_d2 (qual_handle.h), the order is (d2, vertex id) ascending, and nothing
// is ever summed, so ids, votes and the bits of d2 depend on nothing but (positions, train, labels, rows, k).  The host sorts
// the training set by vertex id once, so that a training row's RANK orders as its id does: the kernels compare (d2, rank),
// and a query that is itself a training vertex leaves out its own rank.
//
//   kv_gather_kernel    the training rows, packed (T, D) in rank order
//   kv_select_kernel    one thread per (query row, piece of the training set): the row sits in registers (D = 2 .. 16; other
//                       D read it from memory), the workgroup stages the piece's training rows through LDS in tiles and
//                       every lane reads the same staged row (a broadcast).  The thread keeps its best L entries as a
//                       sorted (d2, rank) list in registers (L = 8, 16 or 32, the least that holds k, else 32): a candidate
//                       is first compared with the worst entry, and an insertion is a fully unrolled compare-and-shift.  A
//                       wave pays for an insertion when any of its lanes inserts, which early in a piece is nearly always:
//                       a short list makes that both rarer and cheaper.  k > 32 takes ceil(k / 32) passes over the piece; a
//                       pass admits only what lies strictly after the last entry of the pass before, so no entry needs a
//                       mark.  After each pass the list goes to the (row, piece) slot of the list array.
//   kv_merge_kernel     one wave per query row, lane p at the head of piece p's list: k wave minima give the row's k
//                       nearest in order; the classes of the taken are kept two to a lane and counted against each other,
//                       O(k^2 / 64) a lane, so a class id needs no bound.  It runs for one piece as for many.
//   lp_round_kernel     one round of label propagation: a wave per vertex, lanes striding the row, a histogram of n_classes
//                       int32 per wave in LDS
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <utility>
#include <vector>

#include "cent_handle.h"
#include "dispatch.h"
#include "host_util.h"
#include "qual_handle.h"

#define KV_MAX_K 128
#define KV_L 32                            // entries of a thread's list at most: 64 registers; 8 and 16 for k up to 8 and 16
#define KV_TILE_ROWS 256                   // training rows of a staged tile at most
#define KV_TILE_FLOATS 4096                // floats of a staged tile: 16 KiB; a tile holds min(256, 4096 / D) rows
#define KV_MAX_PIECES 64                   // one lane of the merging wave per piece
// Fewer row blocks than this and the training set is cut into pieces over gridDim.y.  256 compute units hold two workgroups
// of the 32-entry kernel each (its 176 to 190 registers).  Measured 2026-10-20 on one MI355X with 32-entry lists at k = 10
// (python tools/node_classification.py --blocks 16 --n-per-block 6250 / 62500 --iters 20): a threshold of 512 / 1024 / 2048
// gave 8.5 / 10.3 / 10.7 ms at 100 K vertices (1 / 2 / 2 pieces) and 0.185 / 0.241 / 0.323 s at a million (1 / 2 / 4): every
// piece pays the start of its list again, so pieces are for launches that would otherwise leave compute units idle.
#define KV_MIN_BLOCKS 512
#define KV_BATCH_ENTRIES ((int64_t)1 << 22)  // (rows * list entries) of one launch with one piece: 32 MiB of lists
#define KV_LIST_ENTRIES ((int64_t)1 << 24)   // list entries of one launch over all pieces: 128 MiB
#define KV_NONE 0x7FFFFFFF                 // the rank of an empty list entry: after every candidate, also among +inf
#define KV_MERGE_WAVES (QUAL_BLOCK / 64)

#define LP_MAX_CLASSES 1024
#define LP_WAVES (QUAL_BLOCK / 64)         // vertices a workgroup takes at a time: 16 KiB of histograms
#define LP_MAX_BLOCKS 4096

namespace {

// (d, i) ranks before (e, j)
__host__ __device__ __forceinline__ bool kv_before(float d, int32_t i, float e, int32_t j) { return d < e || (d == e && i < j); }

template <int L> __device__ __forceinline__ void kv_insert(float (&ld)[L], int32_t (&li)[L], float d, int32_t i) {
    // (d, i) is carried down the list: where it ranks before a slot's entry the two change places, and from there on the
    // carried entry is the slot's old one, which ranks before the next.  Each step rewrites one slot in place.
#pragma unroll
    for (int j = 0; j < L; ++j) {
        const bool b = kv_before(d, i, ld[j], li[j]);
        const float td = ld[j];
        const int32_t ti = li[j];
        ld[j] = b ? d : td;
        li[j] = b ? i : ti;
        d = b ? td : d;
        i = b ? ti : i;
    }
}

// dst row j = row ids[j] of the snapshot
__global__ __launch_bounds__(QUAL_BLOCK) void kv_gather_kernel(int64_t total, int D, const float *__restrict__ pos, const int32_t *__restrict__ ids,
                                                               float *__restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * QUAL_BLOCK + threadIdx.x;
    if (i < total) dst[i] = pos[(int64_t)ids[i / D] * D + i % D];
}

struct KvSelect {
    const float *pos, *train;       // the snapshot; the training rows, packed (T, D) in rank order
    const int32_t *rows;            // NULL: row r is vertex r
    const int32_t *rank;            // n: a vertex's rank in the training set, -1 outside it
    float *list_d;                  // (pieces, kpad, stride): entry j of (piece p, local row r) at (p * kpad + j) * stride + r
    int32_t *list_i;
    int64_t T, row0, nr, stride;
    int32_t D, tile_rows, piece_tiles, passes, staged;
};

// Thread t of workgroup blockIdx.x owns the query row row0 + 256 blockIdx.x + t and meets the tiles [blockIdx.y * piece_tiles,
// ...) of the training set.  DT = 0: the query row is read from memory, and with a.staged = 0 (D > KV_TILE_FLOATS) the
// training rows are too.  An idle thread walks row 0 and stores nothing.
template <int DT, int L>
__global__ __launch_bounds__(QUAL_BLOCK) void kv_select_kernel(KvSelect a) {
    __shared__ float s_t[KV_TILE_FLOATS];
    const int D = DT > 0 ? DT : a.D;
    const int64_t local = (int64_t)blockIdx.x * QUAL_BLOCK + threadIdx.x;
    const bool live = local < a.nr;
    const int64_t u = live ? (a.rows ? (int64_t)a.rows[a.row0 + local] : a.row0 + local) : 0;
    const float *row = a.pos + u * D;
    float x[DT > 0 ? DT : 1];
    if (DT > 0) {
#pragma unroll
        for (int d = 0; d < DT; ++d) x[d] = row[d];
    }
    const int32_t self = a.rank[u];
    const int64_t n_tiles = (a.T + a.tile_rows - 1) / a.tile_rows;
    const int64_t t0 = (int64_t)blockIdx.y * a.piece_tiles, t1 = min(n_tiles, t0 + a.piece_tiles);
    const int kpad = a.passes * L;
    float last_d = -1.0f;   // before every candidate: a distance is >= +0
    int32_t last_i = -1;
    for (int ps = 0; ps < a.passes; ++ps) {
        float ld[L];
        int32_t li[L];
#pragma unroll
        for (int j = 0; j < L; ++j) {
            ld[j] = INFINITY;
            li[j] = KV_NONE;
        }
        // the bounds are the workgroup's: every thread makes the same trips and meets the same barriers
        for (int64_t t = t0; t < t1; ++t) {
            const int64_t base = t * a.tile_rows;
            const int m = (int)min((int64_t)a.tile_rows, a.T - base);   // m D <= KV_TILE_FLOATS when staged
            if (DT > 0 || a.staged) {
                __syncthreads();
                for (int i = threadIdx.x; i < m * D; i += QUAL_BLOCK) s_t[i] = a.train[base * D + i];
                __syncthreads();
            }
            for (int c = 0; c < m; ++c) {
                const float d = DT > 0       ? qual_d2_fixed<(DT > 0 ? DT : 1)>(x, s_t + c * DT)
                                : a.staged ? qual_d2(row, s_t + c * D, 1, D)
                                           : qual_d2(row, a.train + (base + c) * D, 1, D);
                const int32_t i = (int32_t)(base + c);
                if (!kv_before(d, i, ld[L - 1], li[L - 1])) continue;   // the common case: one comparison
                if (!kv_before(last_d, last_i, d, i) || i == self) continue;  // taken by an earlier pass; the query itself
                kv_insert<L>(ld, li, d, i);
            }
        }
        last_d = ld[L - 1];   // a list that is not full ends in (+inf, KV_NONE): the next pass admits nothing
        last_i = li[L - 1];
        if (!live) continue;
        const int64_t at = ((int64_t)blockIdx.y * kpad + (int64_t)ps * L) * a.stride + local;
        float *out_d = a.list_d + at;   // one running address each, not L of them in registers
        int32_t *out_i = a.list_i + at;
#pragma unroll
        for (int j = 0; j < L; ++j) {
            *out_d = ld[j];
            *out_i = li[j];
            out_d += a.stride;
            out_i += a.stride;
        }
    }
}

struct KvMerge {
    const float *list_d;
    const int32_t *list_i;
    const int32_t *ids, *labels;    // of the training rows in rank order; labels NULL: no vote
    int32_t *out_i, *pred, *votes;  // (nr, k), nr, nr
    float *out_d;
    int64_t nr, stride;
    int32_t k, kpad, pieces;
};

// Wave w of workgroup blockIdx.x owns the local row 4 blockIdx.x + w; lane p < pieces walks piece p's list from its head.
__global__ __launch_bounds__(QUAL_BLOCK) void kv_merge_kernel(KvMerge a) {
    const int lane = threadIdx.x & 63;
    const int64_t local = (int64_t)blockIdx.x * KV_MERGE_WAVES + (threadIdx.x >> 6);
    if (local >= a.nr) return;   // the same in every lane; no barrier below
    const bool mine = lane < a.pieces;
    const int64_t at = (int64_t)(mine ? lane : 0) * a.kpad * a.stride + local;
    int head = 0;
    float hd = mine ? a.list_d[at] : INFINITY;
    int32_t hi = mine ? a.list_i[at] : KV_NONE;
    int32_t lab0 = -1, lab1 = -1;   // the classes of the taken j = lane and j = 64 + lane
    int m = 0;
    for (int j = 0; j < a.k; ++j) {
        float bd = hd;
        int32_t bi = hi;
        for (int off = 32; off > 0; off >>= 1) {
            const float od = __shfl_xor(bd, off, 64);
            const int32_t oi = __shfl_xor(bi, off, 64);
            if (kv_before(od, oi, bd, bi)) { bd = od; bi = oi; }
        }
        const bool some = bi != KV_NONE;   // the same in every lane
        if (lane == 0) {
            a.out_i[local * a.k + j] = some ? a.ids[bi] : -1;
            a.out_d[local * a.k + j] = some ? bd : INFINITY;
        }
        if (!some) continue;
        m = j + 1;
        if (a.labels) {
            const int32_t c = a.labels[bi];
            if (lane == (j & 63)) { if (j < 64) lab0 = c; else lab1 = c; }
        }
        if (mine && hi == bi) {   // ranks are distinct across the pieces: one lane advances
            ++head;
            hd = head < a.kpad ? a.list_d[at + (int64_t)head * a.stride] : INFINITY;
            hi = head < a.kpad ? a.list_i[at + (int64_t)head * a.stride] : KV_NONE;
        }
    }
    if (!a.labels) return;
    int32_t n0 = 0, n1 = 0;   // how many of the taken share the class of this lane's two
    for (int j = 0; j < m; ++j) {
        const int32_t c = __shfl(j < 64 ? lab0 : lab1, j & 63, 64);
        n0 += c == lab0;
        n1 += c == lab1;
    }
    // the greatest count, then the least class; a lane without a taken neighbour offers (0, -1)
    int32_t bn = lane < m ? n0 : 0, bc = lane < m ? lab0 : -1;
    if (64 + lane < m && (n1 > bn || (n1 == bn && lab1 < bc))) { bn = n1; bc = lab1; }
    for (int off = 32; off > 0; off >>= 1) {
        const int32_t on = __shfl_xor(bn, off, 64), oc = __shfl_xor(bc, off, 64);
        if (on > bn || (on == bn && on > 0 && oc < bc)) { bn = on; bc = oc; }
    }
    if (lane == 0) {
        a.pred[local] = bc;
        a.votes[local] = bn;
    }
}

// ---- label propagation ---------------------------------------------------------------------------------------------------
// A workgroup strides over the vertices, four at a time, wave = vertex: next[v] from cur alone.  The trip count is the
// workgroup's, so every wave meets the same barriers; a wave past the last vertex or on a seed counts nothing.
__global__ __launch_bounds__(QUAL_BLOCK) void lp_round_kernel(int64_t n, int n_classes, const int64_t *__restrict__ ptr, const int32_t *__restrict__ adj,
                                                              const int32_t *__restrict__ seed, const int32_t *__restrict__ cur,
                                                              int32_t *__restrict__ next, int32_t *changed) {
    __shared__ int32_t s_hist[LP_WAVES][LP_MAX_CLASSES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int32_t *hist = s_hist[w];
    for (int64_t base = (int64_t)blockIdx.x * LP_WAVES; base < n; base += (int64_t)gridDim.x * LP_WAVES) {
        const int64_t v = base + w;
        const bool free_v = v < n && seed[v] < 0;   // the same in every lane
        for (int c = lane; c < n_classes; c += 64) hist[c] = 0;
        __syncthreads();
        if (free_v)
            for (int64_t e = ptr[v] + lane; e < ptr[v + 1]; e += 64) {
                const int32_t c = cur[adj[e]];
                if (c >= 0) atomicAdd(&hist[c], 1);
            }
        __syncthreads();
        int32_t bn = 0, bc = -1;   // the greatest count, then the least class
        for (int c = lane; c < n_classes; c += 64) {
            const int32_t cnt = hist[c];
            if (cnt > bn) { bn = cnt; bc = c; }   // c ascends: an equal count later is a greater class
        }
        for (int off = 32; off > 0; off >>= 1) {
            const int32_t on = __shfl_xor(bn, off, 64), oc = __shfl_xor(bc, off, 64);
            if (on > bn || (on == bn && on > 0 && oc < bc)) { bn = on; bc = oc; }
        }
        if (v < n && lane == 0) {
            const int32_t own = cur[v];
            int32_t now = own;
            if (free_v && bn > 0 && !(own >= 0 && hist[own] == bn)) now = bc;
            next[v] = now;
            if (now != own) *changed = 1;   // every writer stores the same value
        }
        __syncthreads();   // the histogram is cleared at the top
    }
}

// ---- k-NN: the host side -------------------------------------------------------------------------------------------------
// The training set in rank (= vertex id) order.
struct KvTrain {
    std::vector<int32_t> ids, labels, rank;   // T, T (empty without labels), n (-1 outside the set)
};

gh_status kv_check_train(gh_qual *h, int64_t n_train, const int32_t *train, const int32_t *train_labels, KvTrain *out) {
    const int64_t n = h->n;
    out->rank.assign((size_t)n, -1);
    std::vector<int32_t> &where = out->rank;   // first the training row of a vertex, then its rank
    for (int64_t i = 0; i < n_train; ++i) {
        const int64_t v = train[i];
        if (v < 0 || v >= n) return qual_invalid(h, "training row " + std::to_string(i) + " has a vertex id outside [0, n)");
        if (where[(size_t)v] >= 0) return qual_invalid(h, "training row " + std::to_string(i) + " repeats vertex " + std::to_string(v));
        where[(size_t)v] = (int32_t)i;
    }
    for (int64_t i = 0; train_labels && i < n_train; ++i)
        if (train_labels[i] < 0) return qual_invalid(h, "label " + std::to_string(i) + " is negative");
    out->ids.reserve((size_t)n_train);
    if (train_labels) out->labels.reserve((size_t)n_train);
    for (int64_t v = 0; v < n; ++v) {
        const int32_t i = where[(size_t)v];
        if (i < 0) continue;
        where[(size_t)v] = (int32_t)out->ids.size();
        out->ids.push_back((int32_t)v);
        if (train_labels) out->labels.push_back(train_labels[i]);
    }
    return GH_OK;
}

void kv_host(const gh_qual *h, const KvTrain &tr, int k, int64_t n_rows, const int32_t *rows, int32_t *neighbors, float *d2, int32_t *pred,
             int32_t *votes) {
    const int D = h->D;
    const float *pos = h->h_pos.data();
    const int64_t T = (int64_t)tr.ids.size();
    qual_host_parallel(n_rows, 1, [=, &tr](int64_t first, int64_t last) {
        std::vector<std::pair<float, int32_t>> cand;   // (d2, rank)
        std::vector<int32_t> cls;
        for (int64_t r = first; r < last; ++r) {
            const int64_t u = rows ? rows[r] : r;
            cand.clear();
            for (int64_t t = 0; t < T; ++t)
                if (tr.ids[(size_t)t] != u) cand.emplace_back(qual_d2(pos + u * D, pos + (int64_t)tr.ids[(size_t)t] * D, 1, D), (int32_t)t);
            const int64_t m = std::min<int64_t>(k, (int64_t)cand.size());
            std::partial_sort(cand.begin(), cand.begin() + m, cand.end(),
                              [](const std::pair<float, int32_t> &a, const std::pair<float, int32_t> &b) {
                                  return kv_before(a.first, a.second, b.first, b.second);
                              });
            for (int64_t j = 0; j < k; ++j) {
                if (neighbors) neighbors[r * k + j] = j < m ? tr.ids[(size_t)cand[(size_t)j].second] : -1;
                if (d2) d2[r * k + j] = j < m ? cand[(size_t)j].first : INFINITY;
            }
            if (!pred && !votes) continue;
            cls.clear();
            for (int64_t j = 0; j < m; ++j) cls.push_back(tr.labels[(size_t)cand[(size_t)j].second]);
            std::sort(cls.begin(), cls.end());
            int32_t best_n = 0, best_c = -1;
            for (size_t b = 0; b < cls.size();) {
                size_t e = b;
                while (e < cls.size() && cls[e] == cls[b]) ++e;
                if ((int32_t)(e - b) > best_n) { best_n = (int32_t)(e - b); best_c = cls[b]; }   // classes ascend: the least wins a tie
                b = e;
            }
            if (pred) pred[r] = best_c;
            if (votes) votes[r] = best_n;
        }
    });
}

gh_status kv_device(gh_qual *h, const KvTrain &tr, bool vote, int k, int64_t n_rows, const int32_t *rows, int32_t *neighbors, float *d2,
                    int32_t *pred, int32_t *votes) {
    const int D = h->D;
    const int64_t n = h->n, T = (int64_t)tr.ids.size();
    const int L = k <= 8 ? 8 : k <= 16 ? 16 : KV_L;   // the instantiations of kv_select_kernel
    const int passes = (k + L - 1) / L, kpad = passes * L;
    const bool staged = D <= KV_TILE_FLOATS;
    const int tile_rows = staged ? std::min(KV_TILE_ROWS, KV_TILE_FLOATS / D) : KV_TILE_ROWS;
    const int64_t n_tiles = (T + tile_rows - 1) / tile_rows;
    // rows per batch: a multiple of the workgroup, rows * kpad list entries (at least as many as the rows * k results)
    const int64_t batch = std::max<int64_t>(QUAL_BLOCK, std::min((n_rows + QUAL_BLOCK - 1) / QUAL_BLOCK * QUAL_BLOCK, KV_BATCH_ENTRIES / kpad));
    const int64_t blocks_max = batch / QUAL_BLOCK;
    // a few rows only: the training set is cut into pieces so that every compute unit has work
    const int64_t pieces_max = std::max<int64_t>(1, std::min<int64_t>({(int64_t)KV_MAX_PIECES, n_tiles, KV_MIN_BLOCKS / blocks_max,
                                                                        KV_LIST_ENTRIES / (batch * kpad)}));
    GH_HIP(hipSetDevice(h->device));
    gh_dev<float> d_train, d_list_d, d_out_d;
    gh_dev<int32_t> d_ids, d_labels, d_rank, d_rows, d_list_i, d_out_i, d_pred, d_votes;
    const size_t list_bytes = 4 * (size_t)(pieces_max * kpad * batch);
    if (!d_train.alloc(4 * (size_t)(T * D)) || !d_ids.alloc(4 * (size_t)T) || (vote && !d_labels.alloc(4 * (size_t)T)) ||
        !d_rank.alloc(4 * (size_t)n) || (rows && !d_rows.alloc(4 * (size_t)n_rows)) || !d_list_d.alloc(list_bytes) || !d_list_i.alloc(list_bytes) ||
        !d_out_d.alloc(4 * (size_t)(batch * k)) || !d_out_i.alloc(4 * (size_t)(batch * k)) || !d_pred.alloc(4 * (size_t)batch) ||
        !d_votes.alloc(4 * (size_t)batch)) {
        h->err = "hipMalloc failed for " + std::to_string(4 * T * (D + 2) + 4 * n + 2 * (int64_t)list_bytes + 8 * batch * (k + 1)) +
                 " bytes of training rows, lists and results";
        return GH_ERR_NOMEM;
    }
    GH_HIP(hipMemcpyAsync(d_ids.p, tr.ids.data(), 4 * (size_t)T, hipMemcpyHostToDevice, h->stream));
    if (vote) GH_HIP(hipMemcpyAsync(d_labels.p, tr.labels.data(), 4 * (size_t)T, hipMemcpyHostToDevice, h->stream));
    GH_HIP(hipMemcpyAsync(d_rank.p, tr.rank.data(), 4 * (size_t)n, hipMemcpyHostToDevice, h->stream));
    if (rows) GH_HIP(hipMemcpyAsync(d_rows.p, rows, 4 * (size_t)n_rows, hipMemcpyHostToDevice, h->stream));
    if (T > 0) {
        kv_gather_kernel<<<dim3(qual_grid(T * D)), dim3(QUAL_BLOCK), 0, h->stream>>>(T * D, D, h->d_pos.p, d_ids.p, d_train.p);
        GH_LAUNCH_CHECK();
    }
    KvSelect s{};
    s.pos = h->d_pos.p; s.train = d_train.p; s.rows = rows ? d_rows.p : nullptr; s.rank = d_rank.p;
    s.list_d = d_list_d.p; s.list_i = d_list_i.p;
    s.T = T; s.stride = batch; s.D = D; s.tile_rows = tile_rows; s.passes = passes; s.staged = staged;
    KvMerge g{};
    g.list_d = d_list_d.p; g.list_i = d_list_i.p; g.ids = d_ids.p; g.labels = vote ? d_labels.p : nullptr;
    g.out_i = d_out_i.p; g.out_d = d_out_d.p; g.pred = d_pred.p; g.votes = d_votes.p;
    g.stride = batch; g.k = k; g.kpad = kpad;
    for (int64_t row0 = 0; row0 < n_rows; row0 += batch) {
        const int64_t nr = std::min(batch, n_rows - row0);
        const int64_t blocks = (nr + QUAL_BLOCK - 1) / QUAL_BLOCK;
        const int64_t want = std::max<int64_t>(1, std::min(pieces_max, KV_MIN_BLOCKS / blocks));
        s.piece_tiles = (int32_t)std::max<int64_t>(1, (n_tiles + want - 1) / want);
        const int64_t pieces = std::max<int64_t>(1, (n_tiles + s.piece_tiles - 1) / s.piece_tiles);   // <= want <= pieces_max
        s.row0 = row0; s.nr = nr;
        const dim3 grid((unsigned)blocks, (unsigned)pieces), block(QUAL_BLOCK);
        gh_dispatch_value<8, 16, KV_L>(L, [&](auto l) {
            constexpr int LT = decltype(l)::value;
            if (!gh_dispatch_dim(D, [&](auto d, auto) { kv_select_kernel<d(), LT><<<grid, block, 0, h->stream>>>(s); }))
                kv_select_kernel<0, LT><<<grid, block, 0, h->stream>>>(s);
        });
        GH_LAUNCH_CHECK();
        g.nr = nr; g.pieces = (int32_t)pieces;
        kv_merge_kernel<<<dim3((unsigned)((nr + KV_MERGE_WAVES - 1) / KV_MERGE_WAVES)), dim3(QUAL_BLOCK), 0, h->stream>>>(g);
        GH_LAUNCH_CHECK();
        if (neighbors) GH_HIP(hipMemcpyAsync(neighbors + row0 * k, d_out_i.p, 4 * (size_t)(nr * k), hipMemcpyDeviceToHost, h->stream));
        if (d2) GH_HIP(hipMemcpyAsync(d2 + row0 * k, d_out_d.p, 4 * (size_t)(nr * k), hipMemcpyDeviceToHost, h->stream));
        if (pred) GH_HIP(hipMemcpyAsync(pred + row0, d_pred.p, 4 * (size_t)nr, hipMemcpyDeviceToHost, h->stream));
        if (votes) GH_HIP(hipMemcpyAsync(votes + row0, d_votes.p, 4 * (size_t)nr, hipMemcpyDeviceToHost, h->stream));
        GH_HIP(hipStreamSynchronize(h->stream));   // the lists and the results are written again by the next batch
    }
    return GH_OK;
}

gh_status lp_run(gh_cent *h, int n_classes, const int32_t *seed_labels, int max_rounds, int32_t *labels, int32_t *rounds, int32_t *converged) {
    const int64_t n = h->n;
    GH_HIP(hipSetDevice(h->device));
    gh_dev<int32_t> d_seed, d_lab[2], d_changed;
    if (!d_seed.alloc(4 * (size_t)n) || !d_lab[0].alloc(4 * (size_t)n) || !d_lab[1].alloc(4 * (size_t)n) || !d_changed.alloc(4)) {
        h->err = "hipMalloc failed for " + std::to_string(12 * n) + " bytes of labels";
        return GH_ERR_NOMEM;
    }
    GH_HIP(hipMemcpyAsync(d_seed.p, seed_labels, 4 * (size_t)n, hipMemcpyHostToDevice, h->stream));
    GH_HIP(hipMemcpyAsync(d_lab[0].p, seed_labels, 4 * (size_t)n, hipMemcpyHostToDevice, h->stream));
    const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(LP_MAX_BLOCKS, (n + LP_WAVES - 1) / LP_WAVES));
    int it = 0, cur = 0;
    bool done = false;
    while (it < max_rounds) {
        int32_t changed = 0;
        GH_HIP(hipMemsetAsync(d_changed.p, 0, 4, h->stream));
        lp_round_kernel<<<dim3(blocks), dim3(QUAL_BLOCK), 0, h->stream>>>(n, n_classes, h->d_ptr.p, h->d_adj.p, d_seed.p, d_lab[cur].p,
                                                                       d_lab[cur ^ 1].p, d_changed.p);
        GH_LAUNCH_CHECK();
        GH_HIP(hipMemcpyAsync(&changed, d_changed.p, 4, hipMemcpyDeviceToHost, h->stream));
        GH_HIP(hipStreamSynchronize(h->stream));
        cur ^= 1;
        ++it;
        if (!changed) { done = true; break; }
    }
    GH_HIP(hipMemcpyAsync(labels, d_lab[cur].p, 4 * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));
    if (rounds) *rounds = it;
    if (converged) *converged = done ? 1 : 0;
    return GH_OK;
}

}  // namespace

extern "C" gh_status gh_qual_knn_vote(gh_qual_handle h, int32_t k, int64_t n_train, const int32_t *train, const int32_t *train_labels,
                                      int64_t n_rows, const int32_t *rows, int32_t *neighbors, float *d2, int32_t *pred, int32_t *votes) {
    if (!h) { qual_set_create_error("handle is NULL"); return GH_ERR_INVALID; }
    if (k < 1 || k > KV_MAX_K) return qual_invalid(h, "k must be in [1, " + std::to_string(KV_MAX_K) + "], got " + std::to_string(k));
    if (h->D < 1) return qual_invalid(h, "no positions were set");
    if (n_train < 0 || (n_train > 0 && !train)) return qual_invalid(h, "n_train must be >= 0 and train given, got " + std::to_string(n_train));
    if (!train_labels && (pred || votes)) return qual_invalid(h, "pred and votes need train_labels");
    if (!rows) n_rows = h->n;
    if (n_rows < 0) return qual_invalid(h, "n_rows must be >= 0, got " + std::to_string(n_rows));
    KvTrain tr;
    GH_TRY_ST(kv_check_train(h, n_train, train, train_labels, &tr));
    for (int64_t r = 0; rows && r < n_rows; ++r)
        if (rows[r] < 0 || rows[r] >= h->n) return qual_invalid(h, "row " + std::to_string(r) + " has a vertex id outside [0, n)");
    GH_TRY_ST(cl_scan(h));
    if (n_rows == 0) return GH_OK;
    if (h->device < 0) {
        kv_host(h, tr, k, n_rows, rows, neighbors, d2, train_labels ? pred : nullptr, train_labels ? votes : nullptr);
        return GH_OK;
    }
    const gh_status st = kv_device(h, tr, train_labels != nullptr, k, n_rows, rows, neighbors, d2, pred, votes);
    if (st != GH_OK) (void)hipStreamSynchronize(h->stream);   // the device buffers are freed on return
    return st;
}

extern "C" gh_status gh_cent_label_propagation(gh_cent_handle h, int32_t n_classes, const int32_t *seed_labels, int32_t max_rounds,
                                               int32_t *labels, int32_t *rounds, int32_t *converged) {
    if (!h) { cent_set_create_error("handle is NULL"); return GH_ERR_INVALID; }
    if (n_classes < 1 || n_classes > LP_MAX_CLASSES) {
        h->err = "n_classes must lie in [1, " + std::to_string(LP_MAX_CLASSES) + "], got " + std::to_string(n_classes);
        return GH_ERR_INVALID;
    }
    if (max_rounds < 0) { h->err = "max_rounds must be >= 0, got " + std::to_string(max_rounds); return GH_ERR_INVALID; }
    if (!seed_labels || !labels) { h->err = "seed_labels or labels is NULL"; return GH_ERR_INVALID; }
    for (int64_t v = 0; v < h->n; ++v)
        if (seed_labels[v] < -1 || seed_labels[v] >= n_classes) {
            h->err = "seed label " + std::to_string(v) + " is outside [-1, n_classes)";
            return GH_ERR_INVALID;
        }
    const gh_status st = lp_run(h, n_classes, seed_labels, max_rounds, labels, rounds, converged);
    if (st != GH_OK) (void)hipStreamSynchronize(h->stream);
    return st;
}
