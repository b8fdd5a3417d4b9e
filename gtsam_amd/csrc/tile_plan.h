// tile_plan.h -- the symbolic half of the reduced-system Cholesky: which 128 x 128 tiles exist, in which order the two schedules take
// them, how contraction lists are cut into pieces.  Pure index arithmetic on the host, once per graph: plain C++17, nothing of the
// runtime (tile_plan.cpp compiles with any host compiler; tests/cpp/test_tile_plan.cpp links it alone).  cholesky.hip and
// chol_dataflow.hip upload what comes out of here; the kernels and the planner share the constants below.
#pragma once
#include <stdint.h>

#include <vector>

namespace gt {

constexpr int kTile = 128;  // dense tile / panel width of the reduced-system Cholesky
constexpr int kTileDoubles = kTile * kTile;
constexpr int kSub = 16;    // granularity of the structural masks of a tile (one MFMA tile: 8 x 8 bits per 128 x 128 tile; DfLists, analysis.hip)

constexpr long long kPieceBase = 4096;   // part_flag = kPieceBase epoch + finished pieces of the tile's contraction (< kPieceBase pieces per tile)
constexpr int kTaskWords = 12;     // words of a task in the device table: I, J, offset / count into the steps, piece r of R, slots of (I, J) and (J, J), lanes and their first scratch slot, the tile's 64-bit sub-tile mask
constexpr int kChainWords = 4;     // words per diagonal tile in the chain kernel's table: slot of (J, J), slot of (J, J-1) or -1, the 64-bit sub-tile mask of (J, J-1)
constexpr int kStepWords = 6;      // words of a contraction step in the device klist: slots of (I, k), (J, k), their two 64-bit sub-tile masks
// XCD-aware tile order of the stream schedule's update lists (cholesky.hip::k_syrk): supertiles of STI x STJ tiles
constexpr int STI = 8, STJ = 4;

// ---- host half of the stream schedule's plan (context.h::CholPlan adds the device copies) ---------------------------------------
// Which 128x128 tiles exist after fill-in, at the granularity of 256-wide column pairs.
struct CholLists {
  int nt = 0;                                   // 128-tiles of the square part (the rhs tile is index nt)
  int64_t n_stored = 0;                         // stored tiles incl. the rhs row: tile q of the stored list lives in slot q of S
  std::vector<int32_t> h_slot;                  // (nt + 1) x nt: tile (I, J) -> its slot in S, -1 = never touched (chol_device.h::SMat)
  int64_t n_exch = 0;                           // tiles of CholPlan::exch (analysis.hip)
  std::vector<int64_t> trsm_off, trsm_cnt;      // per column tile
  std::vector<int64_t> s1_off, s1_cnt, nar_off, nar_cnt, rest_off, rest_cnt;   // per pair: thin update, look-ahead part, rest
  std::vector<int64_t> bwd_off, bwd_cnt;        // per row tile
  // nested dissection: part of every 256-column pair (parts numbered in elimination order, children before parents),
  // parent part (-1: root); updates of a pair whose target columns lie in an ancestor part
  std::vector<int32_t> pair_part, part_parent;
  std::vector<int64_t> anc_off, anc_cnt;
  std::vector<uint8_t> h_fill;                  // the fill structure over column pairs ((np x np) bytes): what plan_stream_pairs builds the SYRK pair lists from
  bool stream_lists = false;                    // `pairs` and the per-pair offsets are built (on first use of the stream schedule: cholesky.hip::ensure_stream_lists)
  int critical_pairs = 0;                       // pairs on the longest leaf-to-root path (= all pairs without parts)
  double flops = 0.0;                           // algorithmic flops of one factorisation over the stored tiles
  double dense_fraction = 1.0;                  // stored lower tiles / all lower tiles
};

// ---- host half of the dataflow schedule's plan (context.h::DfPlan adds the device copies) ----------------------------------------
struct DfLists {
  int nt = 0;
  int64_t n_tasks = 0;                          // bulk tasks: per block column J the diagonal accumulation PD(J), then the tiles (I, J) below, the rhs tile last
  int64_t n_scratch = 0;                        // scratch slots behind the stored tiles of S: the accumulator lanes 1.. of the tiles with very long contraction lists
  std::vector<int32_t> h_has_sub;               // per diagonal tile J: tile (J, J-1) is stored (its update is streamed by the chain kernel)
  int64_t n_flag_words = 0;                     // flag words by slot, the scratch slots of the accumulator lanes included (chol_dataflow.hip::upload_df_plan)
  std::vector<int32_t> h_tasks, h_klist;        // 6 words per task (I, J, offset / count into h_klist, piece r of R) and the contraction lists, in tile coordinates (debug getters, CPU tests)
  // the diagonal tiles by chain workgroup: workgroup w of k_df_chain factors chain_tiles[chain_off[w] .. chain_off[w + 1]) in that order.
  // One slot = two workgroups that alternate; several slots when a nested-dissection ordering gave the factorisation independent parts
  int n_chain = 0;
  std::vector<int32_t> h_chain_off, h_chain_tiles, h_seq;   // h_seq: the order in which the block columns are taken (ticket groups)
  int critical_tiles = 0;                       // diagonal tiles of the longest slot
  double flops = 0.0, dense_fraction = 1.0;
  double flops_executed = 0.0;                  // flops minus the contraction MFMAs skipped on structurally empty 16 x 16 sub-tiles (df_resolve_host / k_df_resolve)
};

// ---- shared ------------------------------------------------------------------------------------------------------------------------
// Symbolic elimination of an n x n lower-triangular boolean structure (row-major bytes; nullptr = dense): the structure with its
// diagonal and its fill.  Column pairs for the stream schedule, tiles for the dataflow schedule.
std::vector<uint8_t> symbolic_fill(int n, const std::vector<uint8_t>* structure);
// the one or two tiles of column pair q, appended to out
inline void tiles_of(int q, int nt, std::vector<int32_t>& out) { out.push_back(2 * q); if (2 * q + 1 < nt) out.push_back(2 * q + 1); }

// ---- stream schedule (cholesky.hip) ------------------------------------------------------------------------------------------------
// What the device gets beside CholLists::h_slot: concatenated TRSM row tiles, backward column tiles by row, the same tiles by column
// (offsets nt + 1, rows descending), every stored tile (I, J) in slot order.
struct CholTables { std::vector<int32_t> rows, bcols, bwd_col_off, bwd_col_rows, stored; };
// pair_struct = lower-triangular boolean structure over 256-wide column pairs ((np x np) row-major bytes, np = ceil(nt / 2); nullptr = dense)
CholTables plan_chol(CholLists& plan, int nt, const std::vector<uint8_t>* pair_struct,
                     const std::vector<int32_t>* pair_part = nullptr, const std::vector<int32_t>* part_parent = nullptr);
// The SYRK pair lists of a plan (from its h_fill): the concatenated (I, J) pairs; fills the per-pair s1 / nar / rest / anc offsets.
std::vector<int32_t> plan_stream_pairs(CholLists& plan);

// ---- dataflow schedule (chol_dataflow.hip): named stages ------------------------------------------------------------------------------
struct TileFill {                                // stage 1: the filled tile structure and its rows
  int nt = 0, bw = 0;                            // bw: 64-bit words of a row's bit set
  std::vector<uint8_t> B;                        // nt x nt
  std::vector<std::vector<int32_t>> rowcols;     // per row tile: its column tiles k < i, ascending
  std::vector<uint64_t> rowbits;                 // the same rows as bit sets: a tile's contraction list is the AND of two of them
};
TileFill df_fill_rows(int nt, const std::vector<uint8_t>* tile_struct);

struct ColumnOrder {                             // stage 2: the order in which the block columns are taken
  bool tree = false;                             // the columns fall into parts (nested dissection)
  int nparts = 1;
  std::vector<int32_t> part_of, seq, pos;        // part of a column; columns in ticket-group order; pos[seq[q]] = q
};
ColumnOrder df_column_sequence(int nt, const std::vector<int32_t>* tile_part, const std::vector<int32_t>* part_parent);

// stage 3: chain slots of the parts and the chain workgroups' lists -> df.h_chain_off, h_chain_tiles, n_chain, critical_tiles, h_seq
void df_chain_lists(DfLists& df, const ColumnOrder& order, const std::vector<int32_t>* part_parent);

struct PieceRec { int32_t I, J, koff, kcnt, r, R; };   // piece r of R of tile (I, J): steps [koff, koff + kcnt) of h_klist
struct Pieces {                                  // stage 4: every tile's contraction list cut into pieces, by place in `seq`
  std::vector<std::vector<PieceRec>> finals, early;   // the last piece of a tile in its own column's group, the early pieces behind their youngest operand
  std::vector<int> diag_last_g;                  // group of the last early piece of PD(J) (-1: none)
};
// -> df.h_klist, h_has_sub, flops, dense_fraction, nt
Pieces df_contraction_pieces(DfLists& df, const TileFill& fill, const ColumnOrder& order);

// stage 5: ticket order with the pull rules -> df.h_tasks, n_tasks
void df_ticket_order(DfLists& df, const Pieces& pieces, bool tree);

// All five in a row.  tile_struct: (nt x nt) row-major bytes, lower triangle: tile (I, J) holds something before the factorisation
// (nullptr = dense); the rhs row (tile row nt) is dense.  GTG_DF_PLAN_TIMING: a line per stage on stderr.
void plan_dataflow(DfLists& df, int nt, const std::vector<uint8_t>* tile_struct,
                   const std::vector<int32_t>* tile_part = nullptr, const std::vector<int32_t>* part_parent = nullptr);

// ---- dataflow schedule: resolved to slots (the device tables) ---------------------------------------------------------------------------
// Accumulator lanes of the tiles with very long contraction lists: 2 words per slot of `slot` (CholLists::h_slot, n_slots stored
// tiles), (lanes G, first of its G - 1 scratch slots behind the stored tiles) or (1, -1).  Sets df.n_scratch.  Read by the host
// resolve below and by k_df_resolve alike.
std::vector<int32_t> df_lane_table(DfLists& df, const std::vector<int32_t>& slot, int64_t n_slots);
struct DfTables { std::vector<int32_t> tasks, steps; double skipped = 0.0; };   // kTaskWords per task, kStepWords per entry of h_klist, flops of the MFMAs left out
// sub16: per tile the 64-bit mask of its 16 x 16 sub-tiles that can be non-zero (analysis.hip; nullptr = all)
DfTables df_resolve_host(const DfLists& df, const std::vector<int32_t>& slot, const std::vector<uint64_t>* sub16, const std::vector<int32_t>& lane_tab);
std::vector<int32_t> df_chain_words(const DfLists& df, const std::vector<int32_t>& slot, const std::vector<uint64_t>* sub16);   // kChainWords per diagonal tile

}  // namespace gt
