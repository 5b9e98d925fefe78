// sgns_api.hip -- the C ABI of skip-gram with negative sampling on a node2vec handle: the four unigram-table builders, the embedding
// tables, the locally-hot key, the slot tables, the two training entry points gemhip_sgns_train / gemhip_sgns_train_part, and the launch knobs.
// It validates, moves data and launches; the small kernels of that set-up live here beside the entry points that launch them.  TrainModel itself
// is sgns.hpp (instantiated in sgns_hogwild.hip, sgns_det.hip, sgns_part.hip); what a launch looks like and what the unigram tables contain is host
// arithmetic without a device (sgns_plan.hip); the handle is n2v_handle.hpp, its graph, walks and counts are n2v.hip's.
#include "sgns.hpp"
#include "n2v_handle.hpp"
#include "n2v_graph.hpp"
#include <hipcub/hipcub.hpp>
#include <vector>
#include <cstring>
#include <cmath>
#include <algorithm>

namespace {

// LOCALLY HOT ROWS (round 6).  wcount[v] = number of walks that CONTAIN v (one wavefront per walk: a token counts at its first occurrence in the walk).
// A node whose tokens are packed into few walks -- count[v] / wcount[v] occurrences per walk that touches it -- sits in that walk's LDS window for the
// whole walk, not for 2R+1 centres: the two nodes of an isolated edge make up ALL 80 tokens of each of their 20 walks.  Two wavefronts that train two of
// those walks at the same time each apply a whole walk's worth of updates (~800 pair steps per row) to the same base and both deltas are added: the pair
// ends with a norm 14 % above its peers' (measured, R-MAT scale 17 at 1 536 wavefronts: profiles/r06_canaries_rmat17.jsonl) and, because the nodes of
// such components are nearly collinear (cosine 0.93; they are only ever pushed away from the same hub rows), outranks the true neighbour of dozens of
// them -- the heavy tail of the power-law "Hogwild bias" (each event costs 2-5 % of the graph's MAP; its probability grows with the width).
__global__ __launch_bounds__(64) void n2v_walk_presence_kernel(const int32_t *__restrict__ walks, int64_t nwalks, int32_t walk_len, int32_t *__restrict__ wcount)
{
    extern __shared__ int32_t tokp[];
    const int lane = threadIdx.x;
    for (int64_t wl = blockIdx.x; wl < nwalks; wl += gridDim.x) {
        const int32_t *walk = walks + wl * walk_len;
        for (int k = lane; k < walk_len; k += WAVE) tokp[k] = walk[k];
        __builtin_amdgcn_wave_barrier();
        for (int k = lane; k < walk_len; k += WAVE) {
            const int32_t v = tokp[k];
            bool first = v >= 0;
            for (int q = 0; q < k && first; ++q) first = tokp[q] != v;
            if (first) atomicAdd(&wcount[v], 1);
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// hotkey[v] = INT32_MAX for a locally hot node (count >= per_walk x walks containing it), else its token count: what the SGNS kernels compare with hot_thr
__global__ void n2v_hotkey_kernel(int64_t n, const int32_t *__restrict__ counts, const int32_t *__restrict__ wcount, int32_t per_walk, int32_t *__restrict__ hotkey,
                                  unsigned int *__restrict__ nlocal)
{
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const int32_t c = counts[v], w = wcount[v];
    const bool loc = w > 0 && (int64_t)c >= (int64_t)per_walk * w;
    hotkey[v] = loc ? INT32_MAX : c;
    if (loc) atomicAdd(nlocal, 1u);
}

// -------------------------------------------------------------------------- SGNS
// InitPosEmb (ELF @0x40e270): (U(0,1)-0.5)/d ; InitNegEmb: zeros.
// first[v] = index of the first token equal to v (LearnVocab @0x40d560 renames the tokens 0..N-1 in that order)
__global__ void n2v_first_token_kernel(const int32_t *__restrict__ walks, int64_t ntokens, unsigned long long *__restrict__ first)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < ntokens; t += stride) {
        const int32_t v = walks[t];
        if (v >= 0 && first[v] > (unsigned long long)t) atomicMin(&first[v], (unsigned long long)t);
    }
}

__global__ void iota_kernel(int32_t *p, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = (int32_t)i;
}

// SgnsArgs::SK.  RndUnigramInt draws slot = floor(u n), X = KT[slot] (quirk) or slot, then reads {UTable[X], KTable[X]}: the second gather depends on
// the first.  SK[slot] = {X, bits of UTable[X], KTable[X], 0} answers both with one 16-byte read (same values: the draws are unchanged bit for bit).
__global__ void n2v_slot_table_kernel(int64_t nslots, const int32_t *__restrict__ KT, const uint2 *__restrict__ UK, int quirk, uint4 *__restrict__ SK)
{
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nslots) return;
    const int32_t X = quirk ? KT[s] : (int32_t)s;
    const uint2 uk = UK[X];
    SK[s] = make_uint4((uint32_t)X, uk.x, uk.y, 0u);
}

__global__ void sgns_init_kernel(float *SynPos, float *SynNeg, int64_t total, int32_t d, uint64_t seed)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t * 4 >= total) return;
    const u32x4 r = philox4x32_10(seed, (uint32_t)t, (uint32_t)((uint64_t)t >> 32), 0u, (uint32_t)TAG_INIT);
    const uint32_t v[4] = {r.x, r.y, r.z, r.w};
    for (int k = 0; k < 4; ++k)
        if (t * 4 + k < total) {
            SynPos[t * 4 + k] = (u01(v[k]) - 0.5f) / (float)d;
            SynNeg[t * 4 + k] = 0.0f;
        }
}
}  // namespace

extern "C" int gemhip_sgns_pairs(gemhip_n2v_t h, int64_t *pairs, int32_t reset)
{
    GEMHIP_REQUIRE(h && pairs, "sgns_pairs: NULL argument");
    GEMHIP_CHECK(hipDeviceSynchronize());
    unsigned long long v = 0;
    GEMHIP_CHECK(hipMemcpy(&v, h->d_pairs, sizeof v, hipMemcpyDeviceToHost));
    if (reset) GEMHIP_CHECK(hipMemset(h->d_pairs, 0, sizeof v));
    *pairs = (int64_t)v;
    return GEMHIP_OK;
}

// ------------------------------------------------------------------ unigram tables
// The four builders below validate, obtain the token counts (and, for the binary's layout, the first-appearance order), call the one host builder
// (sgns_plan.hip build_unigram_tables: Vose per partition, both layouts), upload and commit through the one path (commit_unigram) into their table set --
// the handle's `single` or `parted` -- and copy their optional outputs in the index space gem_hip.h documents for each.  The handle changes only when
// a build succeeds.
static int read_counts(gemhip_n2v_t h, std::vector<int32_t> &cnt)
{
    GEMHIP_CHECK(hipDeviceSynchronize());
    cnt.resize(h->n);
    PhaseScope ph(PH_D2H);
    GEMHIP_CHECK(hipMemcpy(cnt.data(), h->d_counts, h->n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return GEMHIP_OK;
}

static int host_tables(const std::vector<int32_t> &cnt, const int32_t *order, int32_t parts, int32_t flags, UnigramTables &T)
{
    PhaseScope ph(PH_HOST);
    return build_unigram_tables(cnt.data(), (int64_t)cnt.size(), order, parts, flags, T);
}

// {bits of U[i], K[i]} interleaved: one 8-byte gather instead of two 4-byte gathers
static std::vector<uint2> interleave_uk(const std::vector<float> &U, const std::vector<int32_t> &K)
{
    std::vector<uint2> UK(U.size());
    for (size_t i = 0; i < U.size(); ++i) { uint32_t ub; memcpy(&ub, &U[i], 4); UK[i] = make_uint2(ub, (uint32_t)K[i]); }
    return UK;
}

// Uploads T into one table set of the handle and, when every upload succeeded, commits it: the set then describes T, and whatever was derived from
// the previous tables or counts -- the slot table, the hot key -- is stale.  alias_arrays: UT / KT go up too (the single table in the binary's layout
// is read through UK and the slot table only).  Slot entries beyond a partition's slot count go up as 0; never read: a launch draws slots below it.
static int commit_unigram(gemhip_n2v_t h, UnigramSet &S, UnigramTables &T, int32_t parts, bool vocab_order, bool alias_arrays)
{
    {
        PhaseScope ph(PH_H2D);
        const size_t n = T.U.size();
        const std::vector<uint2> uk = interleave_uk(T.U, T.K);
        std::vector<int32_t> Sdev(T.slot);
        for (auto &v : Sdev) if (v < 0) v = 0;
        if (alias_arrays) { GEMHIP_CHECK(S.UT.upload(T.U.data(), n)); GEMHIP_CHECK(S.KT.upload(T.K.data(), n)); }
        GEMHIP_CHECK(S.UK.upload(uk.data(), n));
        if (!Sdev.empty()) GEMHIP_CHECK(S.KTslot.upload(Sdev.data(), n));
    }
    S.vs = std::move(T.vs); S.vs_part = std::move(T.vs_part); S.part_off = T.part_off; S.part_slots = T.part_slots;
    S.parts = parts; S.vocab_order = vocab_order; S.sk_state = -1; h->hotkey_state = 0;
    return GEMHIP_OK;
}

extern "C" int gemhip_n2v_build_unigram(gemhip_n2v_t h, int32_t *counts_out, float *UT_out, int32_t *KT_out)
{
    GEMHIP_REQUIRE(h, "n2v_build_unigram: NULL handle");
    std::vector<int32_t> cnt; UnigramTables T;
    if (int rc = read_counts(h, cnt)) return rc;
    GEMHIP_REQUIRE(host_tables(cnt, nullptr, 1, 0, T) < 0, "n2v_build_unigram: empty vocabulary (no walks?)");
    if (int rc = commit_unigram(h, h->single, T, 1, false, true)) return rc;
    if (counts_out) std::copy(cnt.begin(), cnt.end(), counts_out);
    if (UT_out) std::copy(T.U.begin(), T.U.end(), UT_out);
    if (KT_out) std::copy(T.K.begin(), T.K.end(), KT_out);
    return GEMHIP_OK;
}

// Nodes in order of first appearance in a token buffer on the device (-1 tokens are padding): back[r] = node with the r-th smallest first token index
// (nodes that never occur sort last), cnt = the handle's token counts.  LearnVocab's renaming (ELF @0x40d560) is r -> back[r] over the nodes that occur.
static int first_appearance_order(gemhip_n2v_t h, const int32_t *d_tokens, int64_t ntok, std::vector<int32_t> &back, std::vector<int32_t> &cnt)
{
    // like its sibling builders: the walks / counts may have been produced on a non-blocking stream of the caller (staged C-ABI use); the launches
    // below go to the null stream, which does not wait for such a stream
    GEMHIP_CHECK(hipDeviceSynchronize());
    const int64_t n = h->n;
    GEMHIP_CHECK(h->d_first.reserve(n));
    GEMHIP_CHECK(hipMemset(h->d_first, 0xff, n * sizeof(unsigned long long)));
    hipLaunchKernelGGL(n2v_first_token_kernel, dim3((unsigned)std::min<int64_t>((ntok + 255) / 256, 256 * 16)), dim3(256), 0, 0, d_tokens, ntok, h->d_first);
    GEMHIP_CHECK(hipGetLastError());
    // nodes sorted by their first token index on the device (radix sort of (first, node) pairs: nodes that never occur sort last)
    back.assign(n, 0); cnt.assign(n, 0);
    DevBuf<unsigned long long> keys_out; DevBuf<int32_t> ids; DevBuf<char> tmp; size_t tmp_bytes = 0;
    hipError_t e = keys_out.reserve(n);
    if (e == hipSuccess) e = ids.reserve(2 * n);
    int32_t *ids_out = ids + n;
    if (e == hipSuccess) { hipLaunchKernelGGL(iota_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, ids, n); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, h->d_first.get(), keys_out.get(), ids.get(), ids_out, (int)n);
    if (e == hipSuccess) e = tmp.reserve(tmp_bytes);
    if (e == hipSuccess) e = hipcub::DeviceRadixSort::SortPairs(tmp.get(), tmp_bytes, h->d_first.get(), keys_out.get(), ids.get(), ids_out, (int)n);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) { PhaseScope ph(PH_D2H); e = hipMemcpy(back.data(), ids_out, n * sizeof(int32_t), hipMemcpyDeviceToHost);
                           if (e == hipSuccess) e = hipMemcpy(cnt.data(), h->d_counts, n * sizeof(int32_t), hipMemcpyDeviceToHost); }
    if (e != hipSuccess) return fail(GEMHIP_E_HIP, "first_appearance_order: device sort failed: %s", hipGetErrorString(e));
    return GEMHIP_OK;
}

// InitUnigramTable in the BINARY's layout.  LearnEmbeddings (ELF @0x40ea30) renames the tokens 0..N-1 in order of first appearance in the walk matrix
// (LearnVocab @0x40d560) and builds the alias table over those N entries in that order; RndUnigramInt (@0x40d5f0) then draws a SLOT floor(u N) of that
// table.  Vose's stack discipline makes the table depend on the order of its entries, so the node-id layout of gemhip_n2v_build_unigram is the same
// distribution but not the same table (measured on SBM-1024 with the binary-pinned restatement: -0.33 +- 0.24 % of MAP, profiles/r03_unigram_layout_effect.json).
// Here: first token index per node on the device (atomicMin over the walks), nodes that occur sorted by it (N = their number), Vose over their counts in
// that order, and the result stored in NODE space so that the kernels need no renaming of tokens or tables:
//   KTslot[slot] = node of KTable'[slot]   (flags & 2, the RndUnigramInt quirk; else node of slot)        -- what A.KT points at
//   UK[v]        = {UTable'[r(v)], node of KTable'[r(v)]}   with r(v) the renamed id of node v            -- what A.UK points at
// order_out[N]: node ids in first-appearance order; UT_out / KT_out [N]: the table in RENAMED indices, as the binary holds it (tests compare them
// with oracle/snap_stream.py's).  The walks must be the whole corpus of the handle (single-GPU path).
extern "C" int gemhip_n2v_build_unigram_vocab_order(gemhip_n2v_t h, int32_t flags, int64_t *n_vocab_out, int32_t *order_out, float *UT_out, int32_t *KT_out)
{
    GEMHIP_REQUIRE(h && h->d_walks && h->nwalks > 0, "n2v_build_unigram_vocab_order: no walks");
    std::vector<int32_t> back, cnt; UnigramTables T;             // back: renamed id -> node
    if (int rc = first_appearance_order(h, h->d_walks, h->nwalks * h->walk_len, back, cnt)) return rc;
    GEMHIP_REQUIRE(host_tables(cnt, back.data(), 1, flags, T) < 0, "n2v_build_unigram_vocab_order: empty vocabulary");
    if (int rc = commit_unigram(h, h->single, T, 1, true, false)) return rc;
    const int64_t N = T.n_vocab;
    if (n_vocab_out) *n_vocab_out = N;
    if (order_out) std::copy(back.begin(), back.begin() + N, order_out);
    unigram_table_renamed(h->n, N, back.data(), T.U.data(), T.K.data(), UT_out, KT_out);
    return GEMHIP_OK;
}

// One alias table per partition p = {v : v % parts == p} over local indices v / parts (restricted unigram).
extern "C" int gemhip_n2v_build_unigram_parts(gemhip_n2v_t h, int32_t parts, float *UT_out, int32_t *KT_out)
{
    GEMHIP_REQUIRE(h && parts >= 1 && parts <= h->n, "n2v_build_unigram_parts: bad arguments");
    std::vector<int32_t> cnt; UnigramTables T;
    if (int rc = read_counts(h, cnt)) return rc;
    const int empty = host_tables(cnt, nullptr, parts, 0, T);
    GEMHIP_REQUIRE(empty < 0, "n2v_build_unigram_parts: partition %d has an empty vocabulary", empty);
    if (int rc = commit_unigram(h, h->parted, T, parts, false, true)) return rc;
    if (UT_out) std::copy(T.U.begin(), T.U.end(), UT_out);
    if (KT_out) std::copy(T.K.begin(), T.K.end(), KT_out);
    return GEMHIP_OK;
}

// The per-partition tables in the BINARY's layout (flags bit GEMHIP_N2V_VOCAB_ORDER on the N-GPU schedule): partition p = the nodes v % parts == p that
// occur, in order of first appearance in the whole corpus -- d_corpus: the walks of ALL ranks in walk-id order (rank-major shards, -1 tokens = padding;
// NULL = this handle's own walks: one rank) -- Vose over their counts (the handle's counts: summed over the ranks) in that order; the slot table and the
// alias arrays are stored by LOCAL row v / parts like the node-id layout's.  With one partition this IS gemhip_n2v_build_unigram_vocab_order's table (the same call of the host builder).
// Optional outputs: UT_out / KT_out [n] by local row (concatenated partitions, as the set's UT / KT), slot_out [n] (partition p's slots at part_off[p],
// -1 beyond its slot count), nslots_out [parts].
extern "C" int gemhip_n2v_build_unigram_parts_vocab_order(gemhip_n2v_t h, int32_t parts, int32_t flags, const void *d_corpus, int64_t corpus_tokens,
                                                          float *UT_out, int32_t *KT_out, int32_t *slot_out, int64_t *nslots_out)
{
    GEMHIP_REQUIRE(h && parts >= 1 && parts <= h->n, "n2v_build_unigram_parts_vocab_order: bad arguments");
    GEMHIP_REQUIRE(d_corpus ? corpus_tokens > 0 : (h->d_walks && h->nwalks > 0), "n2v_build_unigram_parts_vocab_order: no walks");
    std::vector<int32_t> back, cnt; UnigramTables T;
    if (int rc = first_appearance_order(h, d_corpus ? (const int32_t *)d_corpus : h->d_walks, d_corpus ? corpus_tokens : h->nwalks * h->walk_len, back, cnt)) return rc;
    const int empty = host_tables(cnt, back.data(), parts, flags, T);
    GEMHIP_REQUIRE(T.n_vocab > 0, "n2v_build_unigram_parts_vocab_order: empty vocabulary");
    GEMHIP_REQUIRE(empty < 0, "n2v_build_unigram_parts_vocab_order: partition %d has an empty vocabulary", empty);
    if (int rc = commit_unigram(h, h->parted, T, parts, true, true)) return rc;
    if (UT_out) std::copy(T.U.begin(), T.U.end(), UT_out);
    if (KT_out) std::copy(T.K.begin(), T.K.end(), KT_out);
    if (slot_out) std::copy(T.slot.begin(), T.slot.end(), slot_out);
    if (nslots_out) std::copy(T.part_slots.begin(), T.part_slots.end(), nslots_out);
    return GEMHIP_OK;
}

extern "C" int gemhip_sgns_init(gemhip_n2v_t h, int32_t d, uint64_t seed, void *dSynPos, void *dSynNeg)
{
    GEMHIP_REQUIRE(h && d >= 1, "sgns_init: bad arguments");
    GEMHIP_REQUIRE(pick_sgns(d) != nullptr, "sgns_init: d=%d unsupported (even d <= 512, odd d <= 256)", d);
    GEMHIP_REQUIRE((dSynPos == nullptr) == (dSynNeg == nullptr), "sgns_init: pass both or neither external table");
    h->syn_own[0].reset(); h->syn_own[1].reset(); h->SynPos = h->SynNeg = nullptr;
    if (!dSynPos) for (auto &b : h->syn_own) GEMHIP_CHECK(b.reserve((size_t)h->n * d));
    h->SynPos = dSynPos ? (float *)dSynPos : h->syn_own[0].get(); h->SynNeg = dSynPos ? (float *)dSynNeg : h->syn_own[1].get();
    h->d = d;
    const int64_t total = h->n * (int64_t)d;
    const int64_t threads = (total + 3) / 4;
    hipLaunchKernelGGL(sgns_init_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, 0, h->SynPos, h->SynNeg, total, d, seed);
    GEMHIP_CHECK(hipGetLastError());
    return GEMHIP_OK;
}

extern "C" int gemhip_sgns_set_tables(gemhip_n2v_t h, const float *SynPos_host, const float *SynNeg_host)
{
    GEMHIP_REQUIRE(h && h->SynPos && SynPos_host && SynNeg_host, "sgns_set_tables: bad arguments (call sgns_init first)");
    const size_t bytes = (size_t)h->n * h->d * sizeof(float);
    GEMHIP_CHECK(hipMemcpy(h->SynPos, SynPos_host, bytes, hipMemcpyHostToDevice));
    GEMHIP_CHECK(hipMemcpy(h->SynNeg, SynNeg_host, bytes, hipMemcpyHostToDevice));
    return GEMHIP_OK;
}

extern "C" int gemhip_sgns_get_tables(gemhip_n2v_t h, float *SynPos_host, float *SynNeg_host)
{
    GEMHIP_REQUIRE(h && h->SynPos, "sgns_get_tables: no tables");
    GEMHIP_CHECK(hipDeviceSynchronize());
    const size_t bytes = (size_t)h->n * h->d * sizeof(float);
    PhaseScope ph(PH_D2H);
    if (SynPos_host) GEMHIP_CHECK(hipMemcpy(SynPos_host, h->SynPos, bytes, hipMemcpyDeviceToHost));
    if (SynNeg_host) GEMHIP_CHECK(hipMemcpy(SynNeg_host, h->SynNeg, bytes, hipMemcpyDeviceToHost));
    return GEMHIP_OK;
}

// LOCALLY HOT ROWS: the array the Hogwild kernels compare with hot_thr -- the token count, or INT32_MAX for a node whose tokens are packed into few walks
// (kernels above).  Built on `stream` from `rows` walks of walk_len tokens (rows of -1 tokens count nothing) and the handle's (possibly externally
// reduced) counts; n_local_hot is read back (one 4-byte copy): a launch without any such node and without count-hot rows keeps the all-cached
// instantiation.  state: what hotkey_state becomes -- 1 built from the handle's own walks, 2 from a gathered corpus.
static int build_hotkey(gemhip_n2v_t h, const int32_t *walks, int64_t rows, int32_t walk_len, hipStream_t stream, int state)
{
    GEMHIP_CHECK(h->d_hotkey.reserve(h->n));
    GEMHIP_CHECK(h->d_wcount.reserve(h->n));
    GEMHIP_CHECK(h->d_nlocal.reserve(1));
    GEMHIP_CHECK(hipMemsetAsync(h->d_wcount, 0, (size_t)h->n * sizeof(int32_t), stream));
    GEMHIP_CHECK(hipMemsetAsync(h->d_nlocal, 0, sizeof(unsigned int), stream));
    if (rows > 0) {
        const int64_t blocks = std::min<int64_t>(rows, 256 * 32);
        hipLaunchKernelGGL(n2v_walk_presence_kernel, dim3((unsigned)blocks), dim3(64), (size_t)walk_len * sizeof(int32_t), stream, walks, rows, walk_len, h->d_wcount);
    }
    hipLaunchKernelGGL(n2v_hotkey_kernel, dim3((unsigned)((h->n + 255) / 256)), dim3(256), 0, stream, h->n, h->d_counts, h->d_wcount, h->kn.local_hot, h->d_hotkey, h->d_nlocal);
    GEMHIP_CHECK(hipGetLastError());
    unsigned int nl = 0;
    GEMHIP_CHECK(hipMemcpyAsync(&nl, h->d_nlocal, sizeof nl, hipMemcpyDeviceToHost, stream));
    GEMHIP_CHECK(hipStreamSynchronize(stream));
    h->n_local_hot = nl;
    h->hotkey_state = state;
    return GEMHIP_OK;
}
// ... of the walks this handle holds: rebuilt after walks / vocabulary change
static int ensure_hotkey(gemhip_n2v_t h, hipStream_t stream)
{
    return h->hotkey_state == 1 ? GEMHIP_OK : build_hotkey(h, h->d_walks, h->nwalks, h->walk_len, stream, 1);
}

// The slot tables the window kernels draw negatives from (SgnsArgs::SK), for the tables the set currently holds and the given quirk bit: partition p's
// slots occupy [part_off[p], part_off[p+1]) of SK, entries in LOCAL rows like KT / UK.  Built on `stream`, in front of the launch that needs them;
// rebuilt only after a table build or when the quirk bit changes.
static int ensure_slot_table(UnigramSet &S, int quirk, hipStream_t stream)
{
    if (S.sk_state == quirk && S.SK) return GEMHIP_OK;
    GEMHIP_CHECK(S.SK.reserve((size_t)S.part_off[S.parts]));
    for (int32_t p = 0; p < S.parts; ++p) {
        const int64_t off = S.part_off[p], np = S.part_slots[p];
        if (np <= 0) continue;
        // (the binary's layout: the slot table names the entry -- quirk already folded in --, the alias arrays are indexed by local row)
        hipLaunchKernelGGL(n2v_slot_table_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, stream, np, (S.vocab_order ? S.KTslot : S.KT) + off,
                           S.UK + off, S.vocab_order ? 1 : quirk, S.SK + off);
    }
    GEMHIP_CHECK(hipGetLastError());
    S.sk_state = quirk;
    return GEMHIP_OK;
}

// The per-wavefront rows of the window kernels: one scratch row each (SgnsArgs::dummy, zeroed when it is allocated) and, for the delta write-back
// of sgns_win_kernel<PART>, the 2R+1 window rows as loaded (SgnsArgs::scratch).  Grow-only: a launch that fits what is held makes no HIP call.
static int ensure_win_scratch(gemhip_n2v_t h, const SgnsLaunchPlan &P, int32_t d, bool part_delta, SgnsArgs &A)
{
    const size_t need = (size_t)P.waves * sgns_win_row_floats(d);
    if (need > h->d_dummy.capacity()) {
        GEMHIP_CHECK(h->d_dummy.reserve(need));
        GEMHIP_CHECK(hipMemset(h->d_dummy, 0, need * sizeof(float)));
    }
    A.dummy = h->d_dummy;
    if (part_delta) GEMHIP_CHECK(h->d_scratch.reserve(need * (size_t)(2 * P.R + 1)));
    A.scratch = part_delta ? h->d_scratch.get() : nullptr;
    return GEMHIP_OK;
}

// Instrumentation builds (scripts/build_variant.sh with -DGEMHIP_SGNS_STALENESS / -DGEMHIP_SGNS_PROFILE): device counters a window launch of
// gemhip_sgns_train carries (begin) and the line printed once it has run (report).  The product build compiles neither.
#ifdef GEMHIP_SGNS_STALENESS
static int staleness_begin(gemhip_n2v_t h, SgnsArgs &A)
{
    static unsigned int *d_sver = nullptr; static unsigned long long *d_shist = nullptr; static int64_t sver_n = 0;
    if (sver_n < h->n) { if (d_sver) hipFree(d_sver); GEMHIP_CHECK(hipMalloc(&d_sver, (size_t)h->n * 2 * sizeof(unsigned int))); sver_n = h->n; }
    if (!d_shist) GEMHIP_CHECK(hipMalloc(&d_shist, 3 * 32 * 16 * sizeof(unsigned long long)));
    GEMHIP_CHECK(hipMemset(d_sver, 0, (size_t)h->n * 2 * sizeof(unsigned int)));
    GEMHIP_CHECK(hipMemset(d_shist, 0, 3 * 32 * 16 * sizeof(unsigned long long)));
    A.stale_ver = d_sver; A.stale_hist = d_shist;
    return GEMHIP_OK;
}
// one JSON line per launch: {"waves", "hot_thr", "fresh", "hist": {class: {log2 count: [launches by bit length of the foreign-update count]}}}
static int staleness_report(gemhip_n2v_t h, const SgnsLaunchPlan &P, const SgnsArgs &A)
{
    std::vector<unsigned long long> hh(3 * 32 * 16);
    GEMHIP_CHECK(hipDeviceSynchronize());
    GEMHIP_CHECK(hipMemcpy(hh.data(), A.stale_hist, hh.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    FILE *fo = getenv("GEMHIP_SGNS_STALENESS_OUT") ? fopen(getenv("GEMHIP_SGNS_STALENESS_OUT"), "a") : stderr;
    if (fo) {
        fprintf(fo, "{\"waves\": %lld, \"hot_thr\": %d, \"fresh\": %d, \"vocab_order\": %d, \"hist\": {", (long long)P.waves, (int)P.hot_thr, (int)A.fresh, (int)h->single.vocab_order);
        const char *cls[3] = {"negative", "centre", "context"};
        for (int c = 0; c < 3; ++c) {
            fprintf(fo, "%s\"%s\": {", c ? ", " : "", cls[c]);
            bool first = true;
            for (int hb = 0; hb < 32; ++hb) {
                unsigned long long tot = 0; for (int sb = 0; sb < 16; ++sb) tot += hh[(c * 32 + hb) * 16 + sb];
                if (!tot) continue;
                fprintf(fo, "%s\"%d\": [", first ? "" : ", ", hb); first = false;
                for (int sb = 0; sb < 16; ++sb) fprintf(fo, "%s%llu", sb ? ", " : "", hh[(c * 32 + hb) * 16 + sb]);
                fprintf(fo, "]");
            }
            fprintf(fo, "}");
        }
        fprintf(fo, "}}\n");
        if (fo != stderr) fclose(fo);
    }
    return GEMHIP_OK;
}
#else
static int staleness_begin(gemhip_n2v_t, SgnsArgs &) { return GEMHIP_OK; }
static int staleness_report(gemhip_n2v_t, const SgnsLaunchPlan &, const SgnsArgs &) { return GEMHIP_OK; }
#endif
#ifdef GEMHIP_SGNS_PROFILE
static int profile_begin(SgnsArgs &A)
{
    static unsigned long long *d_prof = nullptr;
    if (!d_prof) GEMHIP_CHECK(hipMalloc(&d_prof, 64));
    GEMHIP_CHECK(hipMemset(d_prof, 0, 64));
    A.prof = d_prof;
    return GEMHIP_OK;
}
static int profile_report(const SgnsLaunchPlan &P, const SgnsArgs &A)
{
    unsigned long long hp[8];
    GEMHIP_CHECK(hipDeviceSynchronize());
    GEMHIP_CHECK(hipMemcpy(hp, A.prof, 64, hipMemcpyDeviceToHost));
    fprintf(stderr, "[sgns profile] waves=%lld cycles: other=%llu issue=%llu ctx_lds=%llu wait_rows=%llu compute_store=%llu neg_pipeline=%llu centre_setup=%llu centre_end=%llu\n",
            (long long)P.waves, hp[0], hp[1], hp[2], hp[3], hp[4], hp[5], hp[6], hp[7]);
    return GEMHIP_OK;
}
#else
static int profile_begin(SgnsArgs &) { return GEMHIP_OK; }
static int profile_report(const SgnsLaunchPlan &, const SgnsArgs &) { return GEMHIP_OK; }
#endif

// What gemhip_sgns_train and gemhip_sgns_train_part hand the kernels alike (every other field keeps SgnsArgs' default until its entry point sets it): the
// walks and the range of work items, alpha's schedule, the Philox keys, the embedding tables, the handle's pair counter and fresh-row knobs, and the
// unigram table the negatives are drawn from -- table `p` of the set S (the handle's single table: p = 0), in the layout it was built in
static SgnsArgs sgns_args(gemhip_n2v_t h, const UnigramSet &S, int32_t p, const int32_t *walks, int64_t walk_lo, int64_t walk_hi, int32_t walk_len, int32_t window, float alpha0,
                          int64_t denom, int64_t token_offset, int64_t walk_id_offset, int32_t epoch, uint64_t seed, int32_t flags, int32_t d, float *SynPos, float *SynNeg)
{
    SgnsArgs A;
    A.walks = walks; A.walk_lo = walk_lo; A.walk_hi = walk_hi; A.walk_len = walk_len; A.window = window;
    // the kernel computes t = token_offset + wl*walk_len + pos with wl the index of the work item
    A.alpha0 = alpha0; A.denom = denom; A.token_offset = token_offset; A.walk_id_offset = walk_id_offset; A.epoch = epoch;
    A.seed = seed; A.flags = flags; A.d = d;
    const int64_t off = S.part_off[p];
    A.UT = S.UT + off; A.KT = S.KT + off; A.UK = S.UK + off; A.n = (uint32_t)S.part_slots[p];
    if (S.vocab_order) {      // the binary's table layout: slots over the (partition's) nodes that occur, in first-appearance order; the slot table is always consulted
        A.KT = S.KTslot + off; A.flags = flags | 2; A.UT = nullptr;
    }
    A.SynPos = SynPos; A.SynNeg = SynNeg; A.pairs = h->d_pairs;
    A.fresh = h->kn.fresh; A.neg_thr = h->kn.neg_count; A.n_nodes = h->n;
    return A;
}

// The checks both training entry points make of their schedule arguments: 0 when they pass, else the first that fails (1 window, 2 epoch, 3 the token total)
static int bad_schedule_arg(int32_t window, int32_t epoch, int64_t tokens_total)
{
    return !(window >= 1 && window < 16384) ? 1 : !(epoch >= 0 && epoch < 256) ? 2 : !(tokens_total >= 1) ? 3 : 0;
}

// What both training entry points do once their plan P stands: the slot table of the set the negatives come from, the key the kernel compares with the hot
// threshold, the per-wavefront scratch, the record gemhip_sgns_last_launch reads, and the launch.  `who` names the entry point in a refusal; fn: the launcher
// its picker chose (null: d unsupported); local_hot: the plan was made with a hot key that names locally hot nodes.  A bucket launch is A.parts > 0.
static int launch_planned(gemhip_n2v_t h, const char *who, UnigramSet &S, SgnsArgs &A, const SgnsLaunchPlan &P, bool local_hot, sgns_fn fn, hipStream_t stream)
{
    const bool part = A.parts > 0;
    A.nwaves = (int32_t)P.waves; A.cache_radius = P.R;
    if (P.window) {
        if (int rc = ensure_slot_table(S, (A.flags & 2) ? 1 : 0, stream)) return rc;
        A.SK = S.SK + S.part_off[A.word_part];
        // hot rows (sgns_win_kernel): never cached; the launch then takes the instantiation that handles uncached contexts
        A.counts = h->d_counts; A.hot_thr = P.hot_thr;
        // LOCALLY HOT ROWS: the kernel compares `hotkey` (INT32_MAX for a node whose tokens are packed into few walks, else its token count) with the threshold
        if (P.delta && P.waves > 1 && local_hot) A.counts = h->d_hotkey;
        if (int rc = ensure_win_scratch(h, P, A.d, part && P.delta, A)) return rc;
        if (!part) {
            if (int rc = staleness_begin(h, A)) return rc;
            if (int rc = profile_begin(A)) return rc;
        }
    }
    GEMHIP_REQUIRE(fn != nullptr, "%s: d=%d unsupported", who, A.d);
    h->last_plan = P; h->last_fresh = (P.window && P.delta && P.hot_thr > 0) ? A.fresh : 0;
    fn(A, P.blocks, P.threads, P.lds, stream);
    GEMHIP_CHECK(hipGetLastError());
    if (P.window && !part) {
        if (int rc = staleness_report(h, P, A)) return rc;
        if (int rc = profile_report(P, A)) return rc;
    }
    return GEMHIP_OK;
}

extern "C" int gemhip_sgns_train(gemhip_n2v_t h, int32_t window, int32_t neg, float alpha0, int32_t epochs, int32_t epoch,
                                 int64_t walk_lo, int64_t walk_hi, int64_t tokens_total, int64_t token_offset, uint64_t seed,
                                 int32_t flags, void *stream)
{
    GEMHIP_REQUIRE(h && h->SynPos, "sgns_train: call sgns_init first");
    GEMHIP_REQUIRE(h->single.parts == 1, "sgns_train: call n2v_vocab + n2v_build_unigram first");
    GEMHIP_REQUIRE(neg == SGNS_NEG, "sgns_train: neg=%d unsupported (the reference binary fixes NegSamN=5)", neg);
    const int bad = bad_schedule_arg(window, epoch, tokens_total);
    GEMHIP_REQUIRE(bad != 1, "sgns_train: window=%d", window);
    GEMHIP_REQUIRE(epochs >= 1 && epoch < epochs && bad != 2, "sgns_train: epoch %d of %d", epoch, epochs);
    GEMHIP_REQUIRE(0 <= walk_lo && walk_lo <= walk_hi && walk_hi <= h->nwalks, "sgns_train: bad local walk range");
    GEMHIP_REQUIRE(bad != 3, "sgns_train: tokens_total=%lld", (long long)tokens_total);
    if (walk_hi == walk_lo) return GEMHIP_OK;
    UnigramSet &S = h->single;
    SgnsArgs A = sgns_args(h, S, 0, h->d_walks, walk_lo, walk_hi, h->walk_len, window, alpha0, (int64_t)epochs * tokens_total + 1, token_offset, h->walk_id_offset,
                           epoch, seed, flags, h->d, h->SynPos, h->SynNeg);
    A.prefetch = h->kn.prefetch; A.reload = h->kn.reload;
    SgnsKnobs kn_launch = h->kn;
    kn_launch.node_id_layout = !S.vocab_order;
    // LOCALLY HOT ROWS need the WHOLE corpus on this handle (walks-per-node is a property of the corpus: a rank's shard against all-reduced counts would
    // flag everything); Hogwild launches only
    if (!(flags & 4) && h->kn.local_hot > 0 && h->walk_id_offset == 0 && S.vs.total <= (double)h->nwalks * h->walk_len + 0.5) {
        { const int rc = ensure_hotkey(h, (hipStream_t)stream); if (rc) return rc; }
        kn_launch.has_local_hot = h->n_local_hot > 0;
    }
    const SgnsLaunchPlan P = plan_sgns_launch(S.vs, kn_launch, h->n, h->d, window, h->walk_len, walk_hi - walk_lo, flags);
    GEMHIP_REQUIRE(P.lds <= 64 * 1024, "sgns_train: walk_len/window/d too large for LDS staging (%zu bytes)", P.lds);
    return launch_planned(h, "sgns_train", S, A, P, kn_launch.has_local_hot, !P.window ? pick_sgns(h->d) : P.delta ? pick_sgns_win_hogwild(h->d) : pick_sgns_win_det(h->d),
                          (hipStream_t)stream);
}

// The launch plan for the given token counts, without a device: what gemhip_sgns_train would do on a handle with default knobs (tests/test_sgns_plan.py).
extern "C" int gemhip_sgns_plan_launch(const int32_t *counts, int64_t n, int32_t d, int32_t window, int32_t walk_len, int64_t nwalks, int32_t flags,
                                       int32_t *kernel, int32_t *waves, int32_t *hot_threshold, double *n_eff, double *n_eff_cold)
{
    GEMHIP_REQUIRE(counts && n >= 1 && d >= 1 && window >= 1 && walk_len >= 1 && nwalks >= 1, "sgns_plan_launch: bad arguments");
    VocabStats vs;
    vs.build(counts, n);
    SgnsKnobs kn;
    kn.node_id_layout = !(flags & GEMHIP_N2V_VOCAB_ORDER);
    const SgnsLaunchPlan P = plan_sgns_launch(vs, kn, n, d, window, walk_len, nwalks, flags);
    if (kernel) *kernel = P.kernel();
    if (waves) *waves = (int32_t)P.waves;
    if (hot_threshold) *hot_threshold = P.hot_thr;
    if (n_eff) *n_eff = vs.n_eff;
    if (n_eff_cold) *n_eff_cold = P.hot_thr > 0 ? vs.n_eff_cold((double)P.hot_thr) : vs.n_eff;
    return GEMHIP_OK;
}

// One bucket of the partitioned (N-GPU) schedule trained in WALK order: TrainModel over a walk corpus restricted to the pairs whose context lies in
// partition ctx_part (rows of dSynPos_part) and whose centre word lies in partition word_part (rows of dSynNeg_part; negatives drawn from the unigram
// table restricted to word_part).  The corpus may be assembled from several ranks' shards (d_seg: nseg segments, see SgnsArgs::seg); alpha follows
// the index of the token in the work-item order (token_offset + index).  Same kernel, same draws per (walk id, position) as gemhip_sgns_train: with
// parts == 1 it IS gemhip_sgns_train.  Replaces the pair-list pipeline (emit -> bucket -> all-to-all -> sgns_pairs_kernel) of rounds 2-3: what a
// rank needs from the others is their walks (4 bytes per token, once), not pairs (80 bytes per token, every episode), and the order of the pairs
// inside a bucket is the reference's.
extern "C" int gemhip_sgns_train_part(gemhip_n2v_t h, const void *d_walks, int64_t nwalks, int32_t walk_len, const void *d_seg, int32_t nseg,
                                      int64_t seg_len, int64_t walk_id_offset, int32_t window, float alpha0, int64_t alpha_tokens_total,
                                      int64_t token_offset, int32_t epoch, uint64_t seed, int32_t flags, int32_t ctx_part, int32_t word_part,
                                      void *dSynPos_part, void *dSynNeg_part, int32_t d, void *stream)
{
    GEMHIP_REQUIRE(h && h->parted.parts >= 1, "sgns_train_part: call n2v_build_unigram_parts first");
    UnigramSet &S = h->parted;
    GEMHIP_REQUIRE(nwalks >= 0 && (nwalks == 0 || d_walks) && walk_len >= 1 && walk_len < 65536 && dSynPos_part && dSynNeg_part, "sgns_train_part: bad arguments");
    GEMHIP_REQUIRE(ctx_part >= 0 && ctx_part < S.parts && word_part >= 0 && word_part < S.parts, "sgns_train_part: partitions (%d, %d) of %d", ctx_part, word_part, S.parts);
    GEMHIP_REQUIRE(bad_schedule_arg(window, epoch, alpha_tokens_total) == 0, "sgns_train_part: window=%d epoch=%d", window, epoch);
    GEMHIP_REQUIRE(d_seg == nullptr || (nseg >= 1 && seg_len >= 1 && nwalks == (int64_t)nseg * seg_len), "sgns_train_part: nseg=%d seg_len=%lld nwalks=%lld (need nwalks == nseg * seg_len work items)",
                   nseg, (long long)seg_len, (long long)nwalks);
    GEMHIP_REQUIRE((h->n + S.parts - 1) / S.parts < (int64_t)(1 << 29), "sgns_train_part: more than 2^29 rows per partition");
    if (nwalks == 0) return GEMHIP_OK;
    SgnsArgs A = sgns_args(h, S, word_part, (const int32_t *)d_walks, 0, nwalks, walk_len, window, alpha0, alpha_tokens_total + 1, token_offset, walk_id_offset, epoch, seed,
                           flags, d, (float *)dSynPos_part, (float *)dSynNeg_part);
    A.parts = S.parts; A.ctx_part = ctx_part; A.word_part = word_part; A.seg = (const int64_t *)d_seg; A.nseg = nseg; A.seg_len = seg_len;
    VocabStats vs;
    const SgnsKnobs kn = bucket_knobs(h->kn, S.vs_part[word_part], S.vs, S.parts, walk_len, window, flags, !S.vocab_order, h->hotkey_state == 2 && h->n_local_hot > 0, &vs);
    const SgnsLaunchPlan P = plan_sgns_launch(vs, kn, (int64_t)A.n, d, window, walk_len, nwalks, flags);
    GEMHIP_REQUIRE(P.window, "sgns_train_part: d=%d window=%d walk_len=%d do not fit the LDS window kernel", d, window, walk_len);
    return launch_planned(h, "sgns_train_part", S, A, P, kn.has_local_hot, pick_sgns_win_part(d, P.delta), (hipStream_t)stream);
}

namespace {
__global__ void wave_sum6_test_kernel(const float *in, float *out)
{
    const int lane = lane_id();
    float p[6];
    for (int k = 0; k < 6; ++k) p[k] = in[lane * 6 + k];
    out[lane] = wave_sum6(p, lane);
}
}  // namespace

// Building block exposed for its own parity test: in[64][6] partial sums of one wavefront -> out[64], lane l receiving the
// wave total of value (l & 4) ? 4 + (l & 1) : (l & 3).
extern "C" int gemhip_test_wave_sum6(const float *in_host, float *out_host)
{
    GEMHIP_REQUIRE(in_host && out_host, "test_wave_sum6: NULL argument");
    DevBuf<float> d;
    GEMHIP_CHECK(d.reserve(64 * 6 + 64));
    hipError_t e = hipMemcpy(d, in_host, 64 * 6 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) { hipLaunchKernelGGL(wave_sum6_test_kernel, dim3(1), dim3(64), 0, 0, d, d + 64 * 6); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipMemcpy(out_host, d + 64 * 6, 64 * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(GEMHIP_E_HIP, "test_wave_sum6: %s", hipGetErrorString(e));
    return GEMHIP_OK;
}

// ... the same key from a walk CORPUS assembled from every rank's shard (the partitioned N-GPU schedule: gemhip_sgns_train_part trains buckets of it), with
// the handle's -- all-reduced -- token counts: rows of -1 tokens (padding of shorter shards) count nothing.  Bucket launches on this handle then treat the
// locally hot nodes as hot rows (hotkey is indexed by GLOBAL node id, like the counts the bucket kernels read).
extern "C" int gemhip_n2v_locally_hot_corpus(gemhip_n2v_t h, const void *d_corpus, int64_t corpus_rows, int32_t walk_len, int32_t per_walk, int64_t *count, void *stream)
{
    GEMHIP_REQUIRE(h && d_corpus && corpus_rows >= 1 && walk_len >= 1 && per_walk >= -1, "n2v_locally_hot_corpus: bad arguments");
    if (per_walk >= 0) h->kn.local_hot = per_walk;
    h->hotkey_state = 0; h->n_local_hot = 0;
    if (h->kn.local_hot == 0) { if (count) *count = 0; return GEMHIP_OK; }
    // (state 2: gemhip_sgns_train_part uses it; gemhip_sgns_train rebuilds its own from the handle's walks)
    if (int rc = build_hotkey(h, (const int32_t *)d_corpus, corpus_rows, walk_len, (hipStream_t)stream, 2)) return rc;
    if (count) *count = h->n_local_hot;
    return GEMHIP_OK;
}

extern "C" int gemhip_n2v_locally_hot(gemhip_n2v_t h, int32_t per_walk, int64_t *count, int32_t *hotkey_host)
{
    GEMHIP_REQUIRE(h && per_walk >= -1, "n2v_locally_hot: bad arguments");
    GEMHIP_REQUIRE(h->d_walks && h->nwalks > 0, "n2v_locally_hot: no walks on this handle");
    if (per_walk >= 0 && per_walk != h->kn.local_hot) { h->kn.local_hot = per_walk; h->hotkey_state = 0; }
    if (h->kn.local_hot == 0) {            // off: nothing is locally hot, the key is the token count
        if (count) *count = 0;
        if (hotkey_host) GEMHIP_CHECK(hipMemcpy(hotkey_host, h->d_counts, (size_t)h->n * sizeof(int32_t), hipMemcpyDeviceToHost));
        return GEMHIP_OK;
    }
    { const int rc = ensure_hotkey(h, nullptr); if (rc) return rc; }
    if (count) *count = h->n_local_hot;
    if (hotkey_host) GEMHIP_CHECK(hipMemcpy(hotkey_host, h->d_hotkey, (size_t)h->n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return GEMHIP_OK;
}

extern "C" int gemhip_sgns_last_launch(gemhip_n2v_t h, int32_t *kernel, int32_t *waves, int32_t *hot_threshold, int32_t *fresh)
{
    GEMHIP_REQUIRE(h, "sgns_last_launch: null handle");
    const SgnsLaunchPlan &P = h->last_plan;
    if (kernel) *kernel = P.kernel();
    if (waves) *waves = (int32_t)P.waves;
    if (hot_threshold) *hot_threshold = P.hot_thr;
    if (fresh) *fresh = h->last_fresh;
    return GEMHIP_OK;
}

// ------------------------------------------------------------------ launch knobs (per handle; the environment overrides are read once, in gemhip_n2v_create)
extern "C" int gemhip_n2v_set_max_waves(gemhip_n2v_t h, int32_t max_waves)
{
    GEMHIP_REQUIRE(h && max_waves >= 0, "n2v_set_max_waves: bad arguments");
    h->kn.max_waves = max_waves;
    return GEMHIP_OK;
}

extern "C" int gemhip_sgns_set_window_cache(gemhip_n2v_t h, int32_t radius, int32_t delta_writeback)
{
    GEMHIP_REQUIRE(h && radius >= -1 && radius <= 31 && delta_writeback >= -1 && delta_writeback <= 1, "sgns_set_window_cache: bad arguments");
    h->kn.cache_radius = radius;
    h->kn.cache_delta = delta_writeback;
    return GEMHIP_OK;
}

extern "C" int gemhip_sgns_set_hogwild(gemhip_n2v_t h, int32_t prefetch_pairs, int32_t reload_on_update)
{
    GEMHIP_REQUIRE(h && prefetch_pairs >= 0 && prefetch_pairs <= 2 && reload_on_update >= -1 && reload_on_update <= 1, "sgns_set_hogwild: bad arguments");
    if (prefetch_pairs) h->kn.prefetch = prefetch_pairs;
    if (reload_on_update >= 0) h->kn.reload = reload_on_update;
    return GEMHIP_OK;
}

extern "C" int gemhip_sgns_set_hot_rows(gemhip_n2v_t h, int32_t min_count)
{
    GEMHIP_REQUIRE(h && min_count >= -1, "sgns_set_hot_rows: bad arguments");
    h->kn.hot_count = min_count;
    return GEMHIP_OK;
}

extern "C" int gemhip_sgns_set_fresh(gemhip_n2v_t h, int32_t bits)
{
    GEMHIP_REQUIRE(h && bits >= 0 && bits <= 7, "sgns_set_fresh: bits=%d (0..7)", bits);
    h->kn.fresh = bits;
    return GEMHIP_OK;
}
