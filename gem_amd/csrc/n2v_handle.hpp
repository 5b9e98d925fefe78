// n2v_handle.hpp -- struct gemhip_n2v: the state one node2vec handle carries between the calls of the C ABI.  n2v.hip creates and destroys it and owns
// the graph, the alias tables, the walks and the counts; sgns_api.hip owns the unigram tables, the hot key and the embeddings (3.3).
#pragma once
#include "common.hpp"
#include "sgns_plan.hpp"
#include <vector>

namespace gemhip {
// One set of unigram alias tables as a launch draws from it: one table (parts == 1, local row = node id) or one per partition p = {v : v % parts == p},
// local row v / parts, table p at [part_off[p], part_off[p + 1]) of every array.  Filled by the gemhip_n2v_build_unigram* entry points (sgns_api.hip).
struct UnigramSet {
    int32_t parts = 0;                           // 0: no tables (never built, or -- the single table -- the corpus changed since)
    bool vocab_order = false;                    // the binary's layout (slots over the nodes that occur, in first-appearance order), not the node-id layout
    gemhip::DevBuf<float> UT; gemhip::DevBuf<int32_t> KT;     // alias arrays by local row (the single table in the binary's layout is read through UK and KTslot only: not uploaded)
    gemhip::DevBuf<uint2> UK;                    // {bits of UT[i], KT[i]} interleaved: one 8-byte gather instead of two 4-byte gathers
    gemhip::DevBuf<int32_t> KTslot;              // the binary's layout: the slot table of RndUnigramInt in local rows
    // slot table of the window kernels (SgnsArgs::SK): {X, UT[X], KT[X]} by SLOT, built on the device from the arrays above on the first launch after a
    // table build, once per RndUnigramInt-quirk setting (sk_state: -1 stale, else the quirk bit it was built for)
    gemhip::DevBuf<uint4> SK; int sk_state = -1;
    std::vector<int64_t> part_off;               // parts + 1 offsets
    std::vector<int64_t> part_slots;             // slots RndUnigramInt draws from, per partition
    gemhip::VocabStats vs;                       // vocabulary statistics: how concentrated the row traffic is -> plan_sgns_launch ...
    std::vector<gemhip::VocabStats> vs_part;     // ... and those of each partition's rows (launch rule of gemhip_sgns_train_part)
};
}  // namespace gemhip

struct gemhip_n2v {
    int64_t n = 0, nnz = 0;
    int device = 0;
    bool uniform_rows = true;         // every row has equal weights -> no alias tables needed
    gemhip::DevBuf<int64_t> d_row_ptr;
    gemhip::DevBuf<int32_t> d_col;    // columns sorted inside each row
    // walk start nodes: the nodes that occur in the edge list (the reference binary only knows those; an isolated node
    // never reaches it).  start[0..m_start) ascending; walk id r*m_start + j starts at start[perm_r(j)]
    int64_t m_start = 0;
    gemhip::DevBuf<int32_t> d_start;
    gemhip::DevBuf<float> d_w;
    std::vector<int32_t> hub_rows;    // rows with at least ALIAS_HUB_DEG neighbours (n2v_alias_hub_kernel builds their tables: a workgroup per row)
    std::vector<int64_t> hub_off;     // ... and the offset of each one's scratch segment (prefix sum of their degrees)
    gemhip::DevBuf<float> d_U;        // first-order alias tables (per-row segments)
    gemhip::DevBuf<int32_t> d_K;
    // walks
    gemhip::DevBuf<int32_t> d_walks;  // capacity in tokens
    int64_t nwalks = 0;               // local walks held
    int32_t walk_len = 0;
    int64_t walk_id_offset = 0;       // global id of local walk 0
    // vocabulary / unigram
    int32_t *d_counts = nullptr;      // what the kernels read: counts_own's block, or the caller's (gemhip_n2v_bind_counts)
    gemhip::DevBuf<int32_t> counts_own;          // empty while the counts are borrowed
    gemhip::UnigramSet single;        // the table of gemhip_sgns_train (gemhip_n2v_build_unigram / _vocab_order): parts is 1 while it is usable
    gemhip::UnigramSet parted;        // the per-partition tables of gemhip_sgns_train_part (multi-GPU episode schedule)
    gemhip::DevBuf<unsigned long long> d_first;  // first token index of every node (scratch of the binary-layout builders)
    // embeddings
    int32_t d = 0;
    float *SynPos = nullptr, *SynNeg = nullptr;   // what the kernels train: syn_own's blocks, or the caller's tables (gemhip_sgns_init)
    gemhip::DevBuf<float> syn_own[2]; // empty while the tables are borrowed
    gemhip::SgnsKnobs kn;             // launch knobs (setters of sgns_api.hip; environment overrides read once in gemhip_n2v_create)
    gemhip::DevBuf<int32_t> d_hotkey, d_wcount; gemhip::DevBuf<unsigned int> d_nlocal; int hotkey_state = 0; int64_t n_local_hot = 0;   // LOCALLY HOT ROWS (build_hotkey)
    gemhip::SgnsLaunchPlan last_plan; // what the last gemhip_sgns_train / _train_part on this handle actually launched (gemhip_sgns_last_launch)
    int32_t last_fresh = 0;
    gemhip::DevBuf<float> d_dummy;    // sgns_win_kernel: one scratch row per wavefront
    gemhip::DevBuf<float> d_scratch;  // sgns_win_kernel<PART>: the window rows as loaded, 2R+1 rows per wavefront
    gemhip::DevBuf<unsigned long long> d_pairs;  // (centre,context) pairs trained so far
};

// walks, counts or the counts' owner changed: the single table and the hot key of the handle's own walks describe another corpus
inline void corpus_changed(gemhip_n2v *h) { h->single.parts = 0; h->hotkey_state = 0; }
