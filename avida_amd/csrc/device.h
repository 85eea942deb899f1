// device.h -- HBM layout of the organism SoA and device helpers shared by the
// HIP kernels of the batched heads-CPU interpreter (gfx950 / MI355X).
//
// Layout (DESIGN.md "Data layout in HBM"): one organism per cell, structure of
// arrays, every array indexed [field_row * N + cell] so that a wavefront of 64
// consecutive list entries touches 64 consecutive words when the list is in
// cell order.  The memory tape of cell c lives in tape[c * TAPE_SLOT ...] as one
// byte per site: bits 0-5 = canonical handler id (include/avida_gpu.h), bit 6 =
// copied flag, bit 7 = executed flag (cpu/cCPUMemory.h:31-37; the mutated /
// copy-mut flags are statistics only and are not kept on device).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/avida_gpu.h"

#define TAPE_SLOT 2048
// birth record row b_inh[r * BI_WORDS ..]: merit, fitness (doubles), generation,
// copied size, executed size, gestation time, the offspring's RNG key and
// counter, the parent's last task counts; then the record's placement state
// (words 24..31: its parent's cell, the parent's divide number, the offspring's
// length after the divide mutations, its BS_* state (births.h), its target of
// the current round and that round's claim key, 8-B aligned) -- everything a
// placement kernel needs of a record is in the row it loads first
// (BI_FINAL bit 0 = 1: the divide left the offspring's fitness and key and the
// parent's phenotype to finalize_key / finalize_phenotype, place.hip; bits
// 16..31 the offspring's birth time in the update, 1/2^16 -- DESIGN.md 5)
enum { BI_MERIT = 0, BI_FITNESS = 2, BI_GEN = 4, BI_CCOPIED = 5, BI_EXEC = 6, BI_GEST = 7,
       BI_RLO = 8, BI_RHI = 9, BI_RCTR = 10, BI_FINAL = 11, BI_LTASK = 12,
       BI_PARENT = 24, BI_SEQ = 25, BI_LEN = 26, BI_STATE = 27, BI_TARGET = 28, BI_PRIO = 30, BI_WORDS = 32 };
// words 22..23, after the nine task counts (the divide stores them as 0): the
// genotype key of the parent's birth genome (DevWorld::pkey), written by the
// record's round-0 pick -- before any activation of the step can overwrite the
// parent cell's gkey -- and read by activation with the task counts' quad
enum { BI_PKEY = 22 };
static_assert(BI_LTASK + AVGPU_NUM_LOGIC_TASKS <= BI_PKEY && BI_PKEY % 2 == 0 && BI_PKEY + 2 <= BI_PARENT,
              "b_inh row: the parent's genotype key sits in the task quads' spare words, 8-B aligned");
static_assert(BI_LTASK + 12 <= BI_PARENT && BI_PARENT % 4 == 0 && BI_TARGET % 4 == 0 && BI_PRIO % 2 == 0 &&
              BI_PRIO + 2 == BI_WORDS, "b_inh row: the placement words are its last two quads");
#define BI_TIME(w) ((uint32_t)(w) >> 16)
#define CODE_MASK 0x3F
#define TF_COPIED 0x40
#define TF_EXEC 0x80
#define CODE_ERROR 0x3F  /* cInstSet::GetInstError: never a nop */

// ctl word bits
#define CTL_SP0(c) ((c) & 0xF)
#define CTL_SP1(c) (((c) >> 4) & 0xF)
#define CTL_CURSTK 0x100u
#define CTL_MAL 0x200u
#define CTL_ALIVE 0x400u
// "fresh" offspring (k_activate): registers, heads, stacks, label, IO
// buffers, counters, task / reaction counts and bonus hold their birth values
// (zero, default bonus) implicitly -- the SoA rows are stale until the
// organism's first slice writes them back.  Every reader honours the bit.
#define CTL_FRESH 0x800u
// serial world: died in a speculative step (m_spec_die); removed at its next pick
#define CTL_SPECDIE 0x1000u
// head start of an offspring not yet allotted (17 bits: 2^16 - its birth
// time, 1..2^16; 0 = none): its first allotment weights its merit by
// 1 + hs / 2^16 (sched_weight), then clears it
#define CTL_HS_SHIFT 14
#define CTL_HS(c) (((c) >> CTL_HS_SHIFT) & 0x1FFFFu)
#define CTL_HS_MASK (0x1FFFFu << CTL_HS_SHIFT)

#define NUM_CLASSES 4
#define ACLASS_NONE 0xFF
// react_res row: resource slot+1 (0 infinite), spatial?, depletable, type, frac, min, max, value
#define RR_STRIDE 8
enum { RR_RES = 0, RR_SPATIAL = 1, RR_DEPL = 2, RR_TYPE = 3, RR_FRAC = 4, RR_MIN = 5, RR_MAX = 6, RR_VALUE = 7 };
#define RES_FIX 4294967296.0   /* global consumption accumulates in units of 2^-32 */

struct ResParam {
  int32_t geometry, slot;       // slot: row of res_amount (spatial) or -1
  int32_t in_x1, in_x2, in_y1, in_y2, out_x1, out_x2, out_y1, out_y2;
  double in_share;              // inflow / cells of the inflow box (cSpatialResCount::Source)
  double sink_frac;             // 1 - decay, decay = 1 - outflow (cPopulation.cc:440, Sink)
  double xdiffuse, ydiffuse, xgravity, ygravity;
  double decay100, inflow100;   // decay_precalc / inflow_precalc at PRECALC_DISTANCE (global)
  double decay99, inflow99;     // ... at 99 steps (the last block of update 0's 9999 steps)
  int32_t flows, has_sink;      // FlowAll does anything; the outflow box is set
  int32_t in_all, out_all;      // the inflow / outflow box covers every cell exactly once
};
#define NUM_LISTS 7
#define RT_STRIDE 12
enum { RT_TASK = 0, RT_TYPE = 1, RT_MIN = 2, RT_MAX = 3, RT_HASREQ = 4, RT_USED = 5, RT_MULT = 6, RT_ADD = 8 };
// budget bit carried by a slice handed to the next size class: its primary
// birth record is already in use (budgets are < 2^30: avgpu_step checks)
#define BUDGET_PRIM 0x40000000

// Per-cell execution record: the interpreter-private state of one organism
// (the fields only a slice and the state import / export touch), XS_WORDS
// int32 = 256 B per cell, 256-B aligned.  A slice reads and writes it with
// 13 16-byte accesses per lane (words 0..51) instead of ~50 scattered 4-byte
// SoA accesses -- in budget-sorted windows the lanes of a wave are scattered
// cells, and every SoA store was a partial-line HBM write.  A fresh offspring
// (CTL_FRESH) has none of it stored: its birth values are implied.
enum : int {
  XS_REG = 0,      // 3: registers AX BX CX
  XS_HEAD = 3,     // 4: IP, read, write, flow
  XS_RLABEL = 7,   // read_label: len (4b) | nop i at bits 4+2i
  XS_CYCLES = 8,   // cpu_cycles_used
  XS_TIME = 9,     // time_used
  XS_GEST = 10,    // gestation_start
  XS_ERRORS = 11,  // cur errors (faults)
  XS_INBUF = 12,   // 3: input buffer, most recent first
  XS_INTOT = 15,   // inputs received
  XS_INPTR = 16,   // next input index
  XS_OUTBUF = 17,  // last output
  XS_OUTTOT = 18,  // outputs made
  XS_BONUS = 20,   // 2: cur_bonus (double, 8-B aligned)
  XS_TASK = 22,    // 9: cur_task_count of the logic-9 tasks
  XS_STACK = 32,   // 20: stack k entry j at 32 + 10k + j
  XS_REACT = 52,   // 12: cur_reaction_count of reactions 0..11 (12..15 in cur_react rows)
  XS_NREACT = 12,
  XS_WORDS = 64
};

struct DevWorld {
  int64_t n;  // cells
  // --- hot state (registers in the interpreter) ---
  int32_t* xs;        // [n][XS_WORDS] execution records (above)
  uint32_t* ctl;      // [n]  sp0 | sp1<<4 | cur_stack | mal_active | alive
  int32_t* mem_size;  // [n]
  int32_t* max_exec;  // [n]
  int32_t* birth_len; // [n]  genome length at birth (cPhenotype::genome_length)
  uint64_t* gkey;     // [n]  genome key of the birth genome (systematics census)
  uint32_t* rng;      // [3][n] key_lo, key_hi, ctr
  int32_t* budget;    // [n]  instructions left in this update
  // [n] size class k_allot / k_classify_uniform gave the cell's slice this
  // update (0..3, ACLASS_NONE: no slice).  Only those kernels write it: the
  // class-0 launch and k_window_order select their cells by this tag, never by
  // the live mem_size / budget that the list classes running in the same
  // launch rewrite (a list-class slice that divides down to a class-0
  // size must not be picked up by class 0 in the same update).
  uint8_t* aclass;
  uint8_t* tape;      // [n][TAPE_SLOT]
  // --- cold state ---
  int32_t* inputs;    // [3][n] cell inputs
  int32_t* last_task; // [16][n]
  int32_t* cur_react; // [16][n]: rows XS_NREACT.. only (rows 0..11 live in the execution record)
  double* merit;      // [n]
  double* fitness;    // [n]
  double* credit;     // [n]
  int32_t* gest_time; // [n]
  int32_t* num_div;   // [n]
  int32_t* generation;// [n]
  int32_t* copied;    // [n]
  int32_t* child_copied; // [n]
  int32_t* executed;  // [n]
  // --- per-update work lists / queues ---
  // size-class lists: row k = 1..3 the organisms k_allot put in class k,
  // row 3 + k the organisms that spilled into class k during the update
  int32_t* class_list;   // [NUM_LISTS][n]
  int32_t* order;        // [n] class-0 order of a world update: cells of each SORT_WIN window by budget
  int32_t* class_count;  // [CLASS_COUNT_WORDS] entries of each list row
  unsigned long long* counters; // [16] insts, deaths, divides, births, dropped, ...
  // birth records.  Record r < n holds the first offspring that cell r's
  // parent produced in its slice (no atomics in the interpreter loop); records
  // n .. n+ocap-1 hold further offspring of one slice, reserved atomically.
  // Queue entry i < b_count[BQ_PRIMARY] is record b_list[i]; entry
  // b_count[BQ_PRIMARY] + j is record n + j (rec_of below).
  int64_t rcap;       // n + ocap
  int32_t* b_count;   // [BQ_WORDS] (BQ_* below)
  int32_t* b_list;    // [n] primary record ids, appended per wave after the loop
  int32_t* b_len0;    // [rcap]  the child's length before the divide mutations (b_genome holds that child)
  int32_t* b_edit;    // [5][rcap] its divide-mutation edits (interp_core.h edit_word; 0 = none)
  // variable-count divide-mutation edits of record r (only read when
  // seg_any): segment k holds b_pcnt[k][r] edit words from
  // b_subs[b_pofs[k][r]], applied at its place in Divide_DoMutations' order
  // (SEG_* below); b_count[BQ_SUBS] is the arena's fill of this update, scap its size
  int32_t* b_subs;    // [scap]
  int64_t scap;
  int32_t* b_pofs;    // [NSEG][rcap]
  int32_t* b_pcnt;    // [NSEG][rcap]
  // what the offspring of record r inherits (cPhenotype::SetupOffspring,
  // main/cPhenotype.cc:349-447) and the record's placement state (parent,
  // divide number, length, BS_* state, target, claim key), one 128-B row per
  // record (BI_* above): written with 16-B stores at the divide, read with
  // 16-B loads by placement and activation -- as [field][rcap] rows every
  // field was a scattered 4-B access whose line held no other field of the
  // record (primary records sit at their parent's cell id: ~6 % of the rows)
  int32_t* b_inh;     // [rcap][BI_WORDS]
  uint8_t* b_genome;  // [rcap][TAPE_SLOT]
  // placement scratch, n cells + 2 ghost rows (strip tiles, below)
  uint8_t* occ;       // [n + 2X]
  unsigned long long* claim; // [n + 2X]
  unsigned long long* claim2; // [n + 2X] (claim_r[1])
  // placement rounds 0..3 claim into their own arrays (k_place_round,
  // k_tile_round): claim_r[0] = claim, [1] = claim2, [2], [3], [n + 2X] each;
  // all zero between updates (records clear theirs at activation, k_allot
  // round 3's, k_tile_prep the ghost rows)
  unsigned long long* claim_r[4];
  int32_t* b_tgt;     // [4][rcap] the record's target in each placement round it claimed in
  int32_t* owner;     // [n + 2X]  record id, -1 none, REMOTE_OWNER(k, t) won by a halo birth in round k
  uint32_t* killt;    // [n] 2^16 - the earliest birth time of a round-0 pick that kills the cell's
                      // organism, 0 none (placement launch 0 -> the cancellations of launch 0b)
  // the scheduler's tree (k_block_counts -> k_allot): each 256-cell block's
  // share of the update's picks, then the tree's levels (scratch)
  int64_t* blk_count; // [nb]
  double* tree_scr;   // [2 * P] levels of the top tree over the block partials (P = pow2 >= blocks)
  int64_t* tree_cnt;  // [2 * P] their counts
  int64_t tree_cap;   // P of the allocation (strip tiles: >= every strip's blocks)
  int32_t* sdone;     // [n] instructions a spilled slice ran before it spilled (birth times)
  // test-CPU outputs
  uint8_t* t_flags;   // [n][TAPE_SLOT] executed flags snapshot ('+'/'-')
  int32_t* t_flags_len; // [n]
  uint8_t* t_child;   // [n][TAPE_SLOT]
  int32_t* t_child_len; // [n]
  // tables
  int32_t* rand_cum;  // [64] cumulative integer weights
  uint8_t* rand_code; // [64] canonical code of op i
  uint16_t* task_lut; // [256] logic id -> task bitmask
  int n_ops;
  int32_t rand_total;
  uint8_t* rand_lut;  // [256] draw -> canonical code when rand_total <= 256
  int32_t slow_batch;   // parked lanes that trigger the interpreter's slow phase (1..64)
  int32_t nb_slow_batch;  // the same in the newborn pass
  int32_t ioq_slow_batch; // the same in the main pass of the kernels that queue their IO task checks (interp_core.h IOQ)
  int n_react;
  // reactions, RT_STRIDE words each: task, process type, requisite min / max
  // count, has-requisite, in-use, bonus multiplier (f64), bonus addend (f64)
  int32_t* react_tab; // [AVGPU_MAX_REACTIONS][RT_STRIDE]
  // simple environment (reaction i rewards task i; requisites absent, or
  // min_count <= 0 with max_count 1 or unlimited): the IO check is bit logic
  int32_t env_simple;
  uint32_t env_react_mask;   // tasks with a reaction
  uint32_t env_once_mask;    // tasks whose reaction has max_count 1
  uint32_t env_res_mask;     // reactions drawing on a finite resource
  double* task_tab;          // [32]: bonus factor of task t's reaction, then its addend
  // ---- resources (resources.hip; DESIGN.md "Resources") ----
  int32_t n_res, n_cellres, env_resources;   // env_resources: some reaction consumes a resource
  struct ResParam* res_param;   // [AVGPU_MAX_RESOURCES]
  double* res_amount;           // [n_spatial][n] spatial amounts (row = ResParam::slot)
  double* res_delta;            // [res_delta_words(n)] rate scratch of the spatial step
  double* res_global;           // [AVGPU_MAX_RESOURCES] global levels, fixed during an update
  unsigned long long* res_cons; // [AVGPU_MAX_RESOURCES] global consumption of the update, 2^-32 units
  avgpu_cell_resource* res_cells; // [n_cellres] CELL entries (cell ids are global)
  double* react_res;            // [AVGPU_MAX_REACTIONS][RR_STRIDE] resource-bound process settings
  int8_t res_spatial_host[AVGPU_MAX_RESOURCES];   // host-side launch flags
  int8_t res_flows_host[AVGPU_MAX_RESOURCES];
  int8_t res_cells_host[AVGPU_MAX_RESOURCES];     // resource has CELL entries
  int8_t res_grav_host[AVGPU_MAX_RESOURCES];      // resource has gravity on an axis
  double* res_amount_alt;       // [n_spatial][n] the other buffer of the spatial step
  int8_t res_first;             // host: the next update is the first since the load
  int32_t n_spatial;            // spatial resources (rows of res_amount)
  double* rs_send[2];           // strip tiles: [n_spatial][X] first / last row out
  double* rs_recv[2];           //   and the rows above / below in
  uint8_t fill_code;   // code of op 0 (new sites on allocate)
  // config scalars
  int32_t world_x, world_y, geometry;
  int32_t ave_time_slice, slicing;
  int32_t base_merit_method, base_const_merit;
  double default_bonus, size_range, min_copied_lines, min_exe_lines;
  double merit_default_bonus, required_bonus;
  int32_t inherit_merit, require_allocate, alloc_method, max_label_exe;
  int32_t min_genome, max_genome;  // resolved MIN/MAX (>= 8, <= 2048)
  int32_t cfg_min_genome, cfg_max_genome;  // raw MIN_GENOME_SIZE / MAX_GENOME_SIZE
  int32_t death_method, age_limit;
  int32_t prefer_empty, allow_parent, birth_method;
  // P(p) = u < p: counter threshold ceil(p 2^32), and p itself
  // for RECORDED draws
  uint64_t th_copy_mut, th_div_mut, th_div_ins, th_div_del, th_div_slip, th_div_uni;
  double p_copy_mut, p_div_mut, p_div_ins, p_div_del, p_div_slip, p_div_uni;
  // COPY_INS / COPY_DEL / COPY_UNIFORM / COPY_SLIP (SLIP_COPY_MODE 0) of
  // Inst_HeadCopy; copy_ext: any of them non-zero
  uint64_t th_copy_ins, th_copy_del, th_copy_uni, th_copy_slip;
  double p_copy_ins, p_copy_del, p_copy_uni, p_copy_slip;
  int32_t copy_ext;
  uint64_t no_mut_mask;   // NO_MUT_INSTS: handler codes copy mutations leave alone (bit per code)
  // Divide_CheckViable's task / reaction requirements (avgpu_load_env): the
  // required / immunity task (avgpu_task, -1 none), reaction (index, -1
  // none), REQUIRE_SINGLE_REACTION, MAX_UNIQUE_TASK_COUNT; div_req: any set
  int32_t req_task, imm_task, req_react, imm_react, single_react, max_task_cnt, div_req;
  uint64_t th_div_site;   // DIV_MUT_PROB (per-site substitutions on divide)
  double p_div_site;
  uint64_t th_par_site;   // PARENT_MUT_PROB (per-site substitutions in the parent)
  double p_par_site;
  uint64_t th_par_ins, th_par_del;   // PARENT_INS_PROB, PARENT_DEL_PROB (per site, in the parent)
  double p_par_ins, p_par_del;
  double pois_L[5];       // exp(-DIVIDE_POISSON_{SLIP,MUT,INS,DEL,TRANS}_MEAN), 0 = off
  int32_t pois_any;
  uint64_t th_dsite[5];   // DIV_INS_PROB, DIV_DEL_PROB, DIV_UNIFORM_PROB, DIV_SLIP_PROB, DIV_TRANS_PROB
  double p_dsite[5];
  uint64_t th_dtrans;     // DIVIDE_TRANS_PROB
  double p_dtrans;
  int32_t seg_any;        // some variable-count kind is on (b_subs / b_pofs / b_pcnt allocated)
  int32_t slip_fill_mode;
  int32_t trans_fill_mode;
  int32_t slip_copy_mode;   // SLIP_COPY_MODE: 0 the read head jumps, 1 a slip of the whole memory
  // RECORDED mode (avgpu_set_rng_mode): rec_n doubles; rec_off[c] = the start
  // of cell c's organism's segment, -1 = a counter stream.  rec == nullptr:
  // COUNTER mode everywhere (the REC-free interpreter instantiations run).
  const double* rec;
  int64_t rec_n;
  int64_t* rec_off;
  // the serial world (avgpu_run_serial_updates; allocated on its first use):
  // merit sum tree (stree[1] the root, leaves at stree_size + cell), each
  // organism's speculative-step credit, the world's scheduler stream
  double* stree;
  int64_t stree_size;
  int32_t* spec;     // [n]
  uint32_t* grng;    // [3] lo hi ctr: the scheduler's stream (picks)
  uint32_t* sctx;    // [3] lo hi ctr: the context stream (every other draw of the serial world)
  uint8_t* face;     // [n] connection-list rotation of each cell (cPopulationCell::Rotate)
  // recorded serial streams (avgpu_set_serial_streams): the k-th pick / context
  // draw is srec_sched[k] / srec_ctx[k] (the counters grng[2] / sctx[2])
  const double* srec_sched;
  int64_t srec_sched_n;
  const double* srec_ctx;
  int64_t srec_ctx_n;
  uint32_t seed_lo, seed_hi;
  // Strip tiles (multi-GPU, DESIGN.md "Multi-GPU"): this world holds rows
  // [row0, row0+rows) of a world_x x global_rows torus / grid.  When tiled,
  // occ / claim / owner carry two ghost rows after the n cells: [n, n+X) is
  // global row row0-1 (the tile above), [n+X, n+2X) global row row0+rows (the
  // tile below).  Single world: tiled = 0, row0 = 0, rows = global_rows = world_y.
  int32_t row0, global_rows, rows, tiled;
  int64_t cell0;          // row0 * world_x: global id of local cell 0 (RNG keys, priorities)
  // halo buffers per direction d (0: tile above, 1: tile below), registered by
  // the host: halo_bytes(X) = per round parity X u64 claims on the receiver's
  // edge row and X u64 the sender's own claims on its edge row, then X u8
  // edge-row occupancy (place.hip halo_cl / halo_occ)
  uint8_t* h_send[2];
  uint8_t* h_recv[2];
  // birth-record buffers per direction: HaloHdr, X HaloRec, arena of r_arena bytes
  uint8_t* r_send[2];
  uint8_t* r_recv[2];
  int64_t r_arena;
  // (appended, so that the hot fields keep their offsets in the scalar loads)
  int32_t* age;       // [n] cPhenotype::age during the update (k_allot ticks it; -1 injected, 0 born / divided),
                      // kept only when track_age (BIRTH_METHOD 1 / 2, its one consumer on this path)
  int32_t track_age;  // BIRTH_METHOD 1 / 2: the age row is maintained
  // the class-0 order's bucket histogram of each 4096-cell sub-window
  // (k_allot's workgroups write it, k_window_order scans it): [nsub][SORT_BUCKETS]
  int32_t* sub_hist;
  int32_t* e_list;    // BIRTH_METHOD 4 + PREFER_EMPTY: the cells empty at placement start, ascending
  int32_t* e_blk;     // its per-256-cell counts, then their exclusive offsets (e_blk[nb]: the total)
  int32_t* soup_perm; // serial world, BIRTH_METHOD 4: the reference's empty_cell_id_array (0..N-1 at creation)
  int32_t* reaper;    // serial world, BIRTH_METHOD 5: the reaper queue, a ring of reaper_cap cells
  int64_t* reaper_ix; // [0] its rear (oldest) position, [1] one past its front (newest)
  int64_t reaper_cap;
  // the batch step's newborns and sub-steps:
  int32_t* ran;       // [n] instructions each cell's organism ran in this step's main pass (k_allot zeroes)
  double* cons;       // [n_res][n] its depletable consumption in that pass (k_allot zeroes; env_resources)
  long long* sched;   // [SCHED_WORDS] the scheduler's words (SCHED_* below)
  // the sub-step predictor of this step's main pass, sharded by block like
  // the counters (k_block_counts zeroes it): shard s at pacc[s * PACC_STRIDE]
  // (PACC_* below, pacc_sum)
  long long* pacc;
  const double* totals;   // the step's totals (k_block_counts; TOT_* below)
  // [n] the gkey of the parent's cell at the moment of the divide that put the
  // organism here (the key of the parent's birth genome); 0
  // for an injected / restored organism.  Placement and activation write it,
  // the interpreter never touches it.
  uint64_t* pkey;
};
// (the interpreter loads the fields by scalar offset: none may move)
static_assert(sizeof(DevWorld) == 1624 && offsetof(DevWorld, pkey) == 1616, "DevWorld's size; pkey is appended");

// ---------------------------------------------------------------------------
// The scratch vectors the update's kernels and the host hand each other.  Each
// layout is stated here once: kernels, allocations and host copies take their
// slots and sizes from these definitions, never from a number of their own.

// The step totals (avgpu_world::d_totals = W.totals; k_block_counts writes
// them).  A caller's buffer (avgpu_update_totals / avgpu_update_run) holds the
// first TOT_HANDED slots only.
enum {
  TOT_WEIGHT = 0,   // the weight total: this world's own, or every world's handed in
  TOT_ORGS = 1,     // the living organisms, likewise
  TOT_HANDED = 2,   //   (slots a caller hands in / avgpu_update_totals writes)
  TOT_DIV = 2,      // the weight total the allotment divides by
  TOT_UD = 3,       // the update's UD
  TOT_WORDS = 8     // then k_merit_partial's scratch: nb block partials, nb int32 alive counts
};
__host__ __device__ inline int64_t totals_words(int64_t nb) { return TOT_WORDS + 2 * nb; }

// The scheduler's words W.sched
enum {
  SCHED_CARRY = 1,      // this step's pick carry (newborn picks beyond their victims' leftovers, k_activate)
  SCHED_CARRY_REM = 2,  // the carry not yet taken (taken at an update's first step)
  SCHED_UD = 4,         // the update's UD (AVE_TIME_SLICE x the organisms at its first step)
  SCHED_WORDS = 12
};

// A predictor shard's words (W.pacc; PACC_STRIDE words apart)
enum {
  PACC_WEIGHT = 0,   // its weight term (2^-20 mean weights)
  PACC_Q01 = 1,      // its divide counts of quarters 0 | 1 << 32
  PACC_Q23 = 2       // ... of quarters 2 | 3 << 32
};

// A strip's partials vector (avgpu_tile_partials): nb block partials, nb alive
// counts (doubles), then a tail of int64 bits
enum {
  TAIL_PRED = 0,       // its sub-step predictor
  TAIL_CARRY = 1,      // its pick carry
  TAIL_QUARTER0 = 2,   // .. 5: its predictor's divide counts by quarter
  TAIL_WORDS = 6
};
static_assert(TAIL_QUARTER0 + 4 == TAIL_WORDS, "a strip's tail ends with the four quarter counts");
__host__ __device__ inline int64_t tile_tail_off(int64_t nb) { return 2 * nb; }
__host__ __device__ inline int64_t tile_part_stride(int64_t nb) { return tile_tail_off(nb) + TAIL_WORDS; }

// The predictor mailbox (coherent mapped host memory, avgpu_world::h_pred):
// k_place_claim0 of an update's last step writes it, avgpu_run_update polls it
enum {
  PRED_ACC = 0,       // the predictor
  PRED_ORGS = 1,      // the organisms it is relative to
  PRED_DENSEST = 2,   // its densest quarter's divide count
  PRED_SEQ = 3,       // the sequence number, stored last at system scope
  PRED_WORDS = 4
};

// Birth-queue lengths W.b_count
enum {
  BQ_PRIMARY = 0,    // primary records listed in b_list
  BQ_OVERFLOW = 1,   // overflow records used
  BQ_SUBS = 2,       // b_subs entries used
  BQ_PICKED = 3,     // + m: the records that picked in placement round m = 1..3 of a single
                     // world (k_place_round counts them; 0: the next launch has nothing pending)
  BQ_WORDS = 7
};
// Rows of class_list / class_count: LIST_NEWBORN the newborn pass's class-0
// organisms (k_activate), k = 1..3 the organisms k_allot put in class k,
// LIST_SPILL + k those that spilled into class k
enum { LIST_NEWBORN = 0, LIST_SPILL = 3, CLASS_COUNT_WORDS = 8 };
static_assert(NUM_LISTS <= CLASS_COUNT_WORDS, "a length per list row");

// k_res_step's idle lanes store into res_delta past the n cells: a wave's
// worth of junk slots follows them
#define RES_DELTA_TAIL 64
__host__ __device__ inline int64_t res_delta_words(int64_t n) { return n + RES_DELTA_TAIL; }

// The statistics vector (avgpu_world::d_stats; avgpu_stats_vector hands it
// out as doubles): slots 0 .. NPART-1 the organisms' sums (k_stats_partial's
// rows, reduced by k_stats_final), of which the first NUSED carry data; then
// the update's counters and the scheduler's state (k_stats_final); then
// k_stats_partial's rows, [NPART][nb]
enum {
  ST_ORGS = 0,          // living organisms
  ST_MERIT = 1,         // sums over them: merit
  ST_FITNESS = 2,
  ST_GESTATION = 3,
  ST_GENOME_LEN = 4,
  ST_MAX_FITNESS = 5,   // (a maximum, not a sum)
  ST_GENERATION = 6,
  ST_MEM_SIZE = 7,
  ST_TASK0 = 8,         // .. 16: organisms whose last gestation did task t
  NUSED = ST_TASK0 + AVGPU_NUM_LOGIC_TASKS,   // .. NPART - 1: zero
  NPART = 24,
  ST_INSTS = 24,
  ST_DEATHS = 25,
  ST_DIVIDES = 26,
  ST_BIRTHS = 27,
  ST_DROPPED = 28,
  ST_SPILLS = 29,
  ST_CUM_INSTS = 30,    // over every update; ST_CUM_BIRTHS follows it (avgpu_set_clock writes the pair)
  ST_CUM_BIRTHS = 31,
  ST_SLICES = 32,
  ST_LANESTEPS = 33,
  ST_OVERWRITTEN = 34,
  ST_CANCELLED = 35,
  ST_WASTED = 36,
  ST_PRED = 37,         // the sub-step predictor (int64 bits)
  ST_CARRY = 38,        // the pick carry (int64 bits)
  ST_PRED_ORGS = 39,    // the organisms the predictor is relative to
  ST_PRED_DENSEST = 40, // its densest quarter's divide count (int64 bits)
  ST_QUARTER0 = 41,     // .. 44: its divide counts by quarter (int64 bits)
  NSTAT = 45
};
static_assert(NUSED <= NPART, "k_stats_partial's rows");
static_assert(ST_INSTS == NPART, "the counters follow the partial sums");
static_assert(ST_CUM_BIRTHS == ST_CUM_INSTS + 1, "avgpu_set_clock writes the pair");
static_assert(ST_QUARTER0 + 4 == NSTAT, "the statistics vector ends with the four quarter counts");
__host__ __device__ inline int64_t stats_words(int64_t nb) { return NSTAT + (int64_t)NPART * nb; }

// Integer-coded kernel arguments
// k_merit_partial's `reset`: what its block 0 zeroes first
enum {
  RESET_NONE = 0,
  RESET_COUNTS = 1,   // the update's counters, the birth-queue and class-list lengths
  RESET_QUEUES = 2    // a later step of the update: the queue and list lengths only
};
// k_block_counts' `mode` (sched.hip): where the tree's leaves and the totals come from
enum {
  BC_OWN = 0,         // this world's partials and totals
  BC_GATHERED = 1,    // a strip: every strip's gathered partials vectors
  BC_HANDED_IN = 2,   // this world's partials, the totals of every world handed in
  BC_TOTALS_ONLY = 3  // this world's {weight total, organisms} out, nothing else
};
// k_activate's `fused`
enum { ACT_WORLD = 1 /* single world: resolves round 3 itself */, ACT_STRIP = 2 /* strip: its own winners */ };
// launch_tile_place's `phase` (avgpu_tile_place's numbers), in the order of an update
enum { TP_ROUND = 0, TP_CLAIM0 = 3, TP_PACK = 1, TP_ACTIVATE = 2 };
// k_interpret's `sorted_arg` bits
enum {
  KI_SORTED = 1,   // the class-0 sweep follows the budget-sorted windows
  KI_PRED = 2      // a world update's main pass: its slices add the sub-step predictor
};
// owner of a cell won by a neighbouring strip's offspring in round k at birth time t
#define REMOTE_OWNER(k, t) (-2 - ((k) + 4 * (int)(t)))
// halo buffer: per round parity X u64 claims on the receiver's edge row and X
// u64 the sender's own claims on its edge row, X u8 edge-row occupancy, then
// (round 0's picks) X u32 kill times of the sender's picks on the receiver's
// edge row (2^16 - t, max-reduced)
__host__ __device__ inline int64_t halo_kt_off(int x) { return ((int64_t)x * 33 + 3) / 4 * 4; }
__host__ __device__ inline int64_t halo_bytes(int x) { return (halo_kt_off(x) + 4 * (int64_t)x + 15) / 16 * 16; }
struct HaloHdr { int32_t count, arena_used, overflow, pad; };
// one offspring placed across a tile edge (the migrant record of
// cMultiProcessWorld.cc:142-190, restated for strip tiles)
struct HaloRec {
  int32_t col, round, len, gen, ccopied, exec, gest;
  uint32_t rng_lo, rng_hi, rng_ctr;
  int32_t off;
  uint32_t t;         // birth time (owner bookkeeping, head start)
  double merit, fitness;
  int32_t last_task[AVGPU_NUM_LOGIC_TASKS], pad2[3];   // the parent's (SetupOffspring)
};
// pad2[0..1]: the parent's genotype key, low word first (4-B aligned: two words)
static_assert(sizeof(HaloRec) == 112 && offsetof(HaloRec, last_task) == 64 && offsetof(HaloRec, pad2) == 100 &&
              offsetof(HaloRec, merit) == 48 && offsetof(HaloRec, off) == 40, "HaloRec's layout is fixed");
__host__ __device__ inline int64_t record_bytes(int x, int64_t arena) {
  return (int64_t)sizeof(HaloHdr) + (int64_t)x * (int64_t)sizeof(HaloRec) + arena;
}

// variable-count edit segments of a birth record, in the order applied:
// e0 (slip) or, with a data fill (SLIP_FILL_MODE 2 / 3), the one-shot slip as
// a segment, Poisson slips, per-site slips (two words each with a data fill:
// edit, fill offset), translocations (one-shot, Poisson, per site: two words
// each, three with TRANS_FILL_MODE 1; see births.h), e1 (mut), Poisson
// substitutions, e2 (ins), Poisson insertions, e3 (del), Poisson deletions,
// e4 (uniform), per-site substitutions, insertions, deletions, uniform
// mutations.  Data fills (a slip's or translocation's L codes / source
// sites) sit in the same arena, reserved per event.
enum { SEG_OSLIP = 0, SEG_PSLIP, SEG_SSLIP, SEG_TTRANS, SEG_PTRANS, SEG_STRANS, SEG_PMUT, SEG_PINS, SEG_PDEL, SEG_SMUT, SEG_SINS, SEG_SDEL, SEG_SUNI, NSEG };
// The slots of counters[] are the public enum avgpu_counter (avida_gpu.h),
// the one list of them.
// Counters are sharded over NSHARD lines (CNT_STRIDE x u64 each) so that the
// per-wave adds of a 16K-wave launch do not serialise on one L2 address; they
// are cleared every update, and counters[CNT_CUM_BASE + k] accumulates slot k
// over all updates (k_stats_final).
#define NSHARD 64
#define CNT_STRIDE 64
#define CNT_CUM_BASE (NSHARD * CNT_STRIDE)
#define CNT_WORDS (NSHARD * CNT_STRIDE + CNT_STRIDE)
#define PACC_STRIDE 8
// the predictor's word k summed over the shards (a packed pair of 32-bit
// counts sums without carries for worlds below 2^32 organisms)
__device__ __forceinline__ long long pacc_sum(const DevWorld& W, int k) {
  long long s = 0;
  for (int sh = 0; sh < NSHARD; sh++) s += W.pacc[sh * PACC_STRIDE + k];
  return s;
}
// quarter k's divide count
__device__ __forceinline__ long long quarter_count(const DevWorld& W, int k) {
  return (long long)(((unsigned long long)pacc_sum(W, PACC_Q01 + (k >> 1)) >> (32 * (k & 1))) & 0xFFFFFFFFull);
}
__device__ __forceinline__ long long densest_quarter(const DevWorld& W) {
  return max(max(quarter_count(W, 0), quarter_count(W, 1)), max(quarter_count(W, 2), quarter_count(W, 3)));
}
#define CNT_CUM_INSTS (CNT_CUM_BASE + AVGPU_CNT_INSTS)
#define CNT_CUM_BIRTHS (CNT_CUM_BASE + AVGPU_CNT_BIRTHS)
// 1 once this update's counts are in the running sums (k_stats_final); 0 after
// reset_counts_block, which folds them in itself when statistics were skipped
#define CNT_CUM_FLAG (CNT_CUM_BASE + CNT_STRIDE - 1)

__device__ __forceinline__ int queue_len(const DevWorld& W) {
  const int64_t n = (int64_t)W.b_count[BQ_PRIMARY] + (int64_t)min(W.b_count[BQ_OVERFLOW], (int)(W.rcap - W.n));
  return (int)n;
}
__device__ __forceinline__ int64_t rec_of(const DevWorld& W, int64_t i) {
  const int p = W.b_count[BQ_PRIMARY];
  return i < p ? (int64_t)W.b_list[i] : W.n + (i - p);
}

// Stores issued from inside the interpreter loop for write-only data (birth
// records, test-CPU snapshots) that no later instruction of the kernel reads.
// As inline asm they are outside the compiler's s_waitcnt bookkeeping, so no
// loop iteration waits on vmcnt for them: with compiler-visible stores there,
// every following iteration drained all of the wave's outstanding memory
// operations (~3000 cycles under load) before its first LDS read.  expcnt(0)
// lets the data VGPRs be reused immediately.
__device__ __forceinline__ void st_async_u32(void* p, uint32_t v) {
  asm volatile("global_store_dword %0, %1, off\n\ts_waitcnt expcnt(0)" ::"v"(p), "v"(v));
}
__device__ __forceinline__ void st_async_u64(void* p, uint64_t v) {
  asm volatile("global_store_dwordx2 %0, %1, off\n\ts_waitcnt expcnt(0)" ::"v"(p), "v"(v));
}
// global loads on rarely taken paths that wait for their own data, so that
// the compiler's wait bookkeeping sees no load outstanding after them
__device__ __forceinline__ uint32_t ld_sync_u32(const void* p) {
  uint32_t v;
  asm volatile("global_load_dword %0, %1, off\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(p) : "memory");
  return v;
}
__device__ __forceinline__ uint32_t ld_sync_u8(const void* p) {
  uint32_t v;
  asm volatile("global_load_ubyte %0, %1, off\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(p) : "memory");
  return v;
}
// the same without the memory clobber: a read-only table load that orders
// nothing else (it still waits for itself)
__device__ __forceinline__ uint32_t ld_sync_ro_u32(const void* p) {
  uint32_t v;
  asm volatile("global_load_dword %0, %1, off\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(p));
  return v;
}
__device__ __forceinline__ uint32_t ld_sync_ro_u8(const void* p) {
  uint32_t v;
  asm volatile("global_load_ubyte %0, %1, off\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(p));
  return v;
}
// Read-only tables read through the scalar cache (s_load, counted by lgkmcnt):
// a vector load in the interpreter's loop waits on vmcnt, which also counts
// every store the wave still has in flight (the divide's record stores).
typedef const __attribute__((address_space(4))) double const_f64_t;
// p[0] at a wave-uniform address
__device__ __forceinline__ double ld_uniform_f64(const double* p) {
  return *(const_f64_t*)p;
}
// tab[idx] for a per-lane idx: one scalar load per distinct index among the
// active lanes (waterfall)
__device__ __forceinline__ uint32_t sgather_u8(const uint8_t* tab, uint32_t idx) {
  uint32_t out = 0;
  bool todo = true;
  while (todo) {
    const uint32_t u = __builtin_amdgcn_readfirstlane(idx);
    if (idx == u) {
      // the address made explicitly scalar (an "s" operand computed by VALU
      // was otherwise handed over in a VGPR)
      const uint64_t a = (uint64_t)(tab + (u & ~3u));
      // (readfirstlane returns int: each half through uint32_t, no sign extension)
      const uint64_t sa = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(a >> 32)) << 32) |
                          (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a);
      uint32_t w;
      asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(w) : "s"(sa));
      out = (w >> ((u & 3u) * 8u)) & 0xFFu;
      todo = false;
    }
  }
  return out;
}
// one 16-B store of four words (p 16-byte aligned).  A store of more than 8
// bytes leaves a hazard on its data VGPRs: a VALU write to them right after
// the store can change what is stored.  The compiler pads its own stores; an
// asm store must carry the wait states itself (without them the rows came out
// corrupted, nondeterministically).
__device__ __forceinline__ void st_async_b128(void* p, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  const u32x4 v = {a, b, c, d};
  asm volatile("global_store_dwordx4 %0, %1, off\n\ts_waitcnt expcnt(0)\n\ts_nop 2" ::"v"(p), "v"(v));
}
__device__ __forceinline__ void st_async_u8(void* p, uint32_t v) {
  asm volatile("global_store_byte %0, %1, off\n\ts_waitcnt expcnt(0)" ::"v"(p), "v"(v));
}

// ---------------------------------------------------------------------------
// RNG spec: identical arithmetic to the oracle's Stream.
__host__ __device__ __forceinline__ uint32_t lowbias32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
  return x;
}
__device__ __forceinline__ uint32_t rng_next(uint32_t lo, uint32_t hi, uint32_t& ctr) {
  uint32_t a = lowbias32(ctr * 0x9E3779B9U + hi);
  uint32_t b = lowbias32(a ^ lo);
  ++ctr;
  return b;
}
__device__ __forceinline__ uint32_t rng_below(uint32_t lo, uint32_t hi, uint32_t& ctr, uint32_t n) {
  return (uint32_t)(((uint64_t)rng_next(lo, hi, ctr) * n) >> 32);
}
__device__ __forceinline__ bool rng_p(uint32_t lo, uint32_t hi, uint32_t& ctr, uint64_t th) {
  return (uint64_t)rng_next(lo, hi, ctr) < th;
}
__host__ __device__ __forceinline__ void derive_key(uint32_t a_lo, uint32_t a_hi, uint32_t x, uint32_t y,
                                                    uint32_t& lo, uint32_t& hi) {
  lo = lowbias32(lowbias32(x ^ a_lo) + y);
  hi = lowbias32(lowbias32(y ^ a_hi) + x + 0x632BE5ABU);
}

// cHeadCPU::Adjust (cpu/cHeadCPU.cc:27-50)
// Genome key (restated in oracle/oracle.cc and
// avida_amd/systematics.py): words w = 0 .. ceil(len/4)-1 of the birth genome
// in canonical codes (4 sites little-endian, sites >= len zero) each mixed with
// their index, summed mod 2^64, then mixed with the length.  The sum makes it
// wave-parallel: each lane folds the words it copies, one wave_sum finishes.
__device__ __forceinline__ uint64_t gk_mix(uint64_t z) {
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ uint64_t gk_word(uint32_t word, int w, int len) {
  word &= 0x3F3F3F3Fu;
  const int keep = len - 4 * w;                 // sites of this word inside the genome
  if (keep < 4) word &= (1u << (8 * keep)) - 1u;
  return gk_mix(((uint64_t)(w + 1) << 32) | word);
}
__device__ __forceinline__ uint64_t gk_final(uint64_t sum, int len) {
  const uint64_t k = gk_mix(sum ^ ((uint64_t)len * 0x9E3779B97F4A7C15ull));
  return k ? k : 1ull;
}
// serial form over a tape (one lane)
__device__ __forceinline__ uint64_t gk_tape(const uint8_t* t, int len) {
  uint64_t s = 0;
  for (int w = 0; w < (len + 3) / 4; w++) {
    uint32_t v = 0;
    for (int j = 0; j < 4 && 4 * w + j < len; j++) v |= (uint32_t)t[4 * w + j] << (8 * j);
    s += gk_word(v, w, len);
  }
  return gk_final(s, len);
}

__device__ __forceinline__ int head_adjust(int pos, int size) {
  // wave-uniform test first: the common case (every active lane in range)
  // falls through without entering the divergent adjustment
  const bool out = (unsigned)pos >= (unsigned)size;
  if (__builtin_expect(__ballot(out) != 0ull, 0)) {
    if (out) pos = pos < 0 ? 0 : (pos < 2 * size ? pos - size : pos % size);
  }
  return pos;
}
// head_adjust of a position known to lie in [0, size] (one past a valid site)
__device__ __forceinline__ int head_wrap(int pos, int size) {
  return (unsigned)pos < (unsigned)size ? pos : pos - size;
}

// cInstSet::GetRandomInst (cpu/cInstSet.cc:83-88) -> canonical code
__device__ __forceinline__ uint8_t random_code(const DevWorld& W, uint32_t lo, uint32_t hi,
                                               uint32_t& ctr) {
  uint32_t r = rng_below(lo, hi, ctr, (uint32_t)W.rand_total);
  int i = 0;
  while (i < W.n_ops - 1 && W.rand_cum[i] <= (int32_t)r) i++;
  return W.rand_code[i];
}

// 2^x from IEEE adds / multiplies only (Horner on the Taylor series of
// e^(f ln2), f in [0,1), then an exact scale by 2^n): the same bits on the
// device and in the oracle (oracle/oracle.cc det_exp2); within 1 ulp of
// pow(2, x) (cEnvironment::DoProcesses PROCTYPE_POW, main/cEnvironment.cc:1752)
__device__ __forceinline__ double det_exp2(double x) {
  const double n = floor(x);
  const double t = __dmul_rn(__dsub_rn(x, n), 0.6931471805599453094);
  double y = 1.0;
  for (int k = 22; k >= 1; k--) y = __dadd_rn(1.0, __dmul_rn(y, __ddiv_rn(t, (double)k)));
  return ldexp(y, (int)n);
}

__device__ __forceinline__ double pow_int(double q, int64_t n) {
  double r = 1.0, b = q;
  while (n) { if (n & 1) r = __dmul_rn(r, b); b = __dmul_rn(b, b); n >>= 1; }
  return r;
}
// 1/k for k = 1..64 (oracle INV_K)
__constant__ const double INV_K[65] = {0.0,
  1.0 / 1, 1.0 / 2, 1.0 / 3, 1.0 / 4, 1.0 / 5, 1.0 / 6, 1.0 / 7, 1.0 / 8, 1.0 / 9, 1.0 / 10, 1.0 / 11, 1.0 / 12,
  1.0 / 13, 1.0 / 14, 1.0 / 15, 1.0 / 16, 1.0 / 17, 1.0 / 18, 1.0 / 19, 1.0 / 20, 1.0 / 21, 1.0 / 22, 1.0 / 23,
  1.0 / 24, 1.0 / 25, 1.0 / 26, 1.0 / 27, 1.0 / 28, 1.0 / 29, 1.0 / 30, 1.0 / 31, 1.0 / 32, 1.0 / 33, 1.0 / 34,
  1.0 / 35, 1.0 / 36, 1.0 / 37, 1.0 / 38, 1.0 / 39, 1.0 / 40, 1.0 / 41, 1.0 / 42, 1.0 / 43, 1.0 / 44, 1.0 / 45,
  1.0 / 46, 1.0 / 47, 1.0 / 48, 1.0 / 49, 1.0 / 50, 1.0 / 51, 1.0 / 52, 1.0 / 53, 1.0 / 54, 1.0 / 55, 1.0 / 56,
  1.0 / 57, 1.0 / 58, 1.0 / 59, 1.0 / 60, 1.0 / 61, 1.0 / 62, 1.0 / 63, 1.0 / 64};
// Binomial(n, p) from one 32-bit word h (oracle binom_draw: inversion below a
// mean of 6 on the smaller side, else normal with the binomial's skew, z the
// centred, scaled sum of 4 16-bit uniforms)
__device__ __forceinline__ int64_t binom_draw(int64_t n, double p, uint32_t h) {
  if (n <= 0 || !(p > 0.0)) return 0;
  if (p >= 1.0) return n;
  const bool flip = p > 0.5;
  const double pp = flip ? __dsub_rn(1.0, p) : p, q = __dsub_rn(1.0, pp);
  const double mean = __dmul_rn((double)n, pp);
  int64_t k;
  if (mean < 6.0) {
    const double u = __dmul_rn(__dadd_rn((double)h, 0.5), 2.3283064365386962890625e-10);
    const double r = __ddiv_rn(pp, q);
    double f = pow_int(q, n);
    double F = f;
    k = 0;
    while (F < u && k < n && k < 64) {
      f = __dmul_rn(__dmul_rn(f, __dmul_rn((double)(n - k), r)), INV_K[k + 1]);
      k++;
      F = __dadd_rn(F, f);
    }
  } else {
    uint32_t x = lowbias32(h + 0x9E3779B9U);
    uint32_t sum = (x & 0xFFFFu) + (x >> 16);
    x = lowbias32(x + 0x9E3779B9U);
    sum += (x & 0xFFFFu) + (x >> 16);
    const double z = __dmul_rn(__dsub_rn(__dmul_rn(__dadd_rn((double)sum, 2.0), 1.52587890625e-05), 2.0),
                               1.7320508075688772);
    const double sd = __dsqrt_rn(__dmul_rn(mean, q));   // IEEE, correctly rounded (oracle std::sqrt)
    const double skew = __dmul_rn(__dmul_rn(__dsub_rn(q, pp), __dsub_rn(__dmul_rn(z, z), 1.0)), 0.16666666666666666);
    const double v = __dadd_rn(__dadd_rn(__dadd_rn(mean, __dmul_rn(sd, z)), skew), 0.5);
    k = v < 1.0 ? 0 : (int64_t)floor(v);
    if (k > n) k = n;
  }
  return flip ? n - k : k;
}
// the word of scheduler-tree node `node` in update u (oracle node_draw)
#define SALT_TOP 0x7A11C0DEu
#define SALT_BLOCK 0x51CEB10Cu
#define SALT_NEWBORN 0x4E3B0A17u
__device__ __forceinline__ uint32_t node_draw(uint32_t slo, uint32_t shi, uint32_t update, uint32_t salt,
                                              uint64_t node) {
  return lowbias32(lowbias32(lowbias32(update * 0x85EBCA6BU + shi) ^ (uint32_t)node ^ salt) +
                   (uint32_t)(node >> 32) + slo);
}
// the word of cell `cell` (its global id, below 2^32) in the population event
// `key` (avida_amd/popevents.py event_draw): stateless like
// node_draw, no organism's stream moves.  event_base is the part every cell of
// an event shares (the host computes it once); lowbias32 is a bijection, so
// within one event no two cells draw the same word.
#define SALT_EVENT 0x0E7E47D5u
__host__ __device__ __forceinline__ uint32_t event_base(uint32_t slo, uint32_t shi, uint64_t key) {
  const uint32_t a = lowbias32((uint32_t)(key >> 32) * 0x85EBCA6BU + shi);
  const uint32_t b = lowbias32(a ^ (uint32_t)key ^ SALT_EVENT);
  return lowbias32(b + slo);
}
__host__ __device__ __forceinline__ uint32_t event_draw(uint32_t base, uint64_t cell) {
  return lowbias32(base ^ (uint32_t)cell);
}
// a merit the scheduler can weigh: finite and not negative (NaN, -x and inf
// are never scheduled; large finite merits of multiplicative environments are)
__device__ __forceinline__ bool merit_ok(double m) { return m >= 0.0 && m <= 1.7976931348623157e308; }
// the scheduler weight of a living organism (oracle sched_weight): the same
// in k_merit_partial's partials and k_allot's leaves; at most 2^990, so that
// the scheduler's sums over up to 2^33 organisms stay finite
#define WEIGHT_CAP 0x1p990
__device__ __forceinline__ double sched_weight(double merit, uint32_t ctl) {
  if (!merit_ok(merit)) return 0.0;
  const uint32_t hs = CTL_HS(ctl);
  const double w = hs ? __dmul_rn(merit, __dadd_rn(1.0, __dmul_rn((double)hs, 1.0 / 65536.0))) : merit;
  return merit_ok(w) ? fmin(w, WEIGHT_CAP) : 0.0;
}

// CalcSizeMerit (main/cPhenotype.cc:1760-1816)
__device__ __forceinline__ int size_merit(int method, int base_const, int glen, int copied, int exe) {
  int s;
  switch (method) {
    case 1: return copied;
    case 2: return exe;
    case 3: return glen;
    case 4: s = glen; if (s > copied) s = copied; if (s > exe) s = exe; return s;
    case 5: s = glen; if (s > copied) s = copied; if (s > exe) s = exe;
            return (int)sqrt((double)s);
    default: return base_const;
  }
}
__device__ __forceinline__ int calc_size_merit(const DevWorld& W, int glen, int copied, int exe) {
  return size_merit(W.base_merit_method, W.base_const_merit, glen, copied, exe);
}
// An organism injected into cell c, whose tape already holds its len sites in
// canonical codes: cPopulation::Inject / ActivateOrganism +
// cPhenotype::SetupInject (main/cPhenotype.cc:599-640).  in3: the cell's three
// inputs, or NULL for the test-CPU constants (deterministic) or a draw from
// the cell's stream.  One lane per cell; k_set_orgs and the landscape's seed
// kernels (landscape.hip) both initialise an organism through it.
__device__ __forceinline__ void inject_org(const DevWorld& W, int64_t c, int len, double merit, const int32_t* in3,
                                           int deterministic) {
  const int64_t N = W.n;
  const uint8_t* t = W.tape + c * TAPE_SLOT;
  // registers, heads, label, counters, buffers, task counts, stacks: zero
  int32_t* x = W.xs + c * XS_WORDS;
  for (int k = 0; k < XS_WORDS; k++) x[k] = 0;
  W.ctl[c] = CTL_ALIVE;
  W.mem_size[c] = len;
  int mx = 0;
  if (W.death_method > 0) {                 // cOrganism::initialize (main/cOrganism.cc:216-236)
    mx = W.age_limit;
    if (W.death_method == 2) mx *= len;
    if (mx < 1) mx = 1;
  }
  W.max_exec[c] = mx;
  W.birth_len[c] = len;
  if (W.track_age) W.age[c] = -1;          // injected between updates: age 0 during the next one
  W.gkey[c] = gk_tape(t, len);
  W.pkey[c] = 0ull;                         // no parent: injected
  // stream key (DESIGN.md RNG spec)
  uint32_t lo, hi, ctr = 0;
  derive_key(W.seed_lo, W.seed_hi, (uint32_t)(W.cell0 + c), 0xA5A5A5A5U, lo, hi);
  int in0, in1, in2;
  if (in3) { in0 = in3[0]; in1 = in3[1]; in2 = in3[2]; }
  else if (deterministic) { in0 = 0x0f13149f; in1 = 0x3308e53e; in2 = 0x556241eb; }
  else {                                      // cEnvironment::SetupInputs random
    in0 = (15 << 24) + (int)rng_below(lo, hi, ctr, 1u << 24);
    in1 = (51 << 24) + (int)rng_below(lo, hi, ctr, 1u << 24);
    in2 = (85 << 24) + (int)rng_below(lo, hi, ctr, 1u << 24);
  }
  W.rng[c] = lo; W.rng[N + c] = hi; W.rng[2 * N + c] = ctr;
  if (W.rec_off) W.rec_off[c] = -1;   // a new organism draws from its counter stream
  if (W.spec) W.spec[c] = 0;           // serial world: no speculative credit yet
  W.inputs[c] = in0; W.inputs[N + c] = in1; W.inputs[2 * N + c] = in2;
  W.budget[c] = 0;
  for (int k = 0; k < AVGPU_MAX_REACTIONS; k++) {
    W.last_task[k * N + c] = 0; W.cur_react[k * N + c] = 0;   // record words: zeroed above
  }
  // cPhenotype::SetupInject (main/cPhenotype.cc:599-640)
  *reinterpret_cast<double*>(x + XS_BONUS) = W.default_bonus;
  W.merit[c] = merit > 0.0 ? merit : (double)len;
  W.fitness[c] = 0.0;
  W.credit[c] = 0.0;
  W.gest_time[c] = 0; W.num_div[c] = 0; W.generation[c] = 0;
  W.copied[c] = len; W.child_copied[c] = 0; W.executed[c] = len;
}

// a value the compiler must keep (in an SGPR, or spilled) rather than
// re-load from its invariant source at each use
#define OPQ(x) asm("" : "+s"(x))

__device__ __forceinline__ void count_add(const DevWorld& W, int slot, unsigned long long v) {
  atomicAdd(&W.counters[(blockIdx.x & (NSHARD - 1)) * CNT_STRIDE + slot], v);
}

// LDS size classes of k_interpret (bytes of tape per lane)
// (a block of class S uses 64 x tape_stride(S) B of LDS for tapes; class 0
// holds nothing else: 64 x 320 B = 20 KiB, so 8 one-wave blocks fill a CU's
// 160 KiB -- as many as its ~216 VGPRs admit.  A 316-B stride (79 dwords:
// equal offsets of the 64 lanes in 64 banks) cut the bank conflicts from 47
// to 22 % of LDS cycles but needs dword LDS-DMA staging: class 0 1.12 ->
// 1.50 ms per launch, A/B on one box, profiles/r04c_*).  A split
// slot -- 208 sites in LDS, the rest in the HBM tape, 13 KiB per wave -- for 3
// waves per SIMD was bit-exact but slower, 1.36 against 1.02 ms: 3 waves cap
// the kernel at 168 VGPRs and the spills land in the loop (profiles/r04k_*)
#define CLASS0_SIZE 320
#define CLASS1_SIZE 768
#define CLASS2_SIZE 1536
#define CLASS3_SIZE 2048
__device__ __forceinline__ int class_of(int need) {
  return need <= CLASS0_SIZE ? 0 : (need <= CLASS1_SIZE ? 1 : (need <= CLASS2_SIZE ? 2 : 3));
}
// tape capacity an organism may need this slice: its memory, or the size
// h-alloc would grow it to when it has not allocated yet
__device__ __forceinline__ int need_of(int m, uint32_t ctl, double size_range) {
  if (ctl & CTL_MAL) return m;
  const int grown = m + min((int)(size_range * m), AVGPU_MAX_GENOME - m);
  return grown > m ? grown : m;
}

// ---------------------------------------------------------------------------
// host-side launchers (defined next to their kernels)
// a tuning knob of the environment: its integer value when set and within
// [lo, hi], else dflt (callers cache it per call site)
static inline int env_int(const char* name, int dflt, int lo, int hi) {
  const char* e = getenv(name);
  const int v = e ? atoi(e) : dflt;
  return (v >= lo && v <= hi) ? v : dflt;
}
// the blocks of b threads that cover n items
static inline unsigned nblk(int64_t n, int b) { return (unsigned)((n + b - 1) / b); }

// ---- serial.hip: one update of the serial world ----
// dW: device copy of W (avgpu_world::push_world)
void launch_serial_update(const DevWorld& W, const DevWorld* dW, hipStream_t s);

// ---- interp.hip: the interpreter's launches (its kernels: interp_launch.h) ----
// class 0 runs densely over cells [first, first+count); classes 1..3 over their lists
// after_class[k] (optional): event recorded after the class-k launch
// sorted: a world update's main pass (class 0 follows k_window_order's windows)
void launch_interpret_classes(const DevWorld& W, const DevWorld* dW, int mode, hipStream_t s,
                              int64_t first, int64_t count, int* launches,
                              hipEvent_t* after_class = nullptr, bool sorted = false);
// class-0 windows: k_allot's budgets sorted (descending) inside windows of
// SORT_WIN cells, so that a wave's 64 organisms get similar time slices
#define SORT_WIN 32768
// k_window_order's buckets: budgets 0 .. SORT_BUCKETS-3 (larger ones share the
// last of them), then one bucket for the window's cells that are not class 0
#define SORT_BUCKETS 258
bool class_timing_all();   // AVGPU_CLASS_TIMING (interp.hip)
// the newborn pass of a batch step: the organisms k_activate listed
void launch_newborns(const DevWorld& W, const DevWorld* dW, hipStream_t s);

// ---- state.hip: organisms and their state in and out ----
void launch_classify_uniform(const DevWorld& W, hipStream_t s, int64_t first, int64_t count,
                             const int32_t* d_budget, int32_t uniform);
void launch_set_orgs(const DevWorld& W, hipStream_t s, int64_t first, int64_t count,
                     const uint8_t* d_codes, const int32_t* d_offsets, const int32_t* d_lens,
                     const double* d_merits, const int32_t* d_inputs, int deterministic);
void launch_get_states(const DevWorld& W, hipStream_t s, int64_t first, int64_t count,
                       avgpu_cpu_state* d_states, uint8_t* d_codes, int cap);
void launch_set_states(const DevWorld& W, hipStream_t s, int64_t first, int64_t count, const avgpu_cpu_state* in,
                       const uint8_t* codes, int cap);
void launch_state_digest(const DevWorld& W, hipStream_t s, int64_t first, int64_t count, uint64_t* d_out);
void launch_get_census(const DevWorld& W, hipStream_t s, int64_t first, int64_t count, avgpu_census* d_out);
void launch_get_parent_keys(const DevWorld& W, hipStream_t s, int64_t first, int64_t count, uint64_t* d_out);

// ---- sched.hip: the merit total, the scheduler tree, the allotment ----
void launch_reset_counts(const DevWorld& W, hipStream_t s);
void launch_age_tick(const DevWorld& W, hipStream_t s);
void launch_merit_total(const DevWorld& W, hipStream_t s, double* d_totals, double* d_scratch);
// sub-update `sub` of `nsub` (avgpu_cfg.sub_updates): the
// resources step and the update's counters are reset at sub 0 only; the key
// of the scheduler's node draws is update x nsub + sub (the caller's `update`)
// own_totals: the picks come from this world's own totals (k_block_counts
// BC_OWN); else from the totals handed in in d_totals' TOT_WEIGHT, TOT_ORGS (avgpu_update_totals
// + an all-reduce of every world's {total weight, organisms}), this world's
// share by cMultiProcessWorld's formula (BC_HANDED_IN)
void launch_world_begin(const DevWorld& W, hipStream_t s, double* d_totals, double* d_scratch, uint32_t update,
                        int sub, int nsub, bool own_totals);
// a sub-update's share of the update's picks n (oracle sub_share)
__host__ __device__ __forceinline__ long long sub_share(long long n, int s, int K) {
  return K == 1 ? n : (n * (s + 1)) / K - (n * s) / K;
}
// strip tiles: the partials every strip gathers, then the tree over them
void launch_tile_partials(const DevWorld& W, hipStream_t s, double* d_out, int reset);
void launch_tile_pre(const DevWorld& W, hipStream_t s, const double* d_gathered, int ntiles, double* d_totals,
                     uint32_t update, int sub = 0, int nsub = 1);
// allotment draw of organism (lo, hi) in update u (oracle allot_draw)
__device__ __forceinline__ uint32_t allot_draw(uint32_t lo, uint32_t hi, uint32_t update) {
  return lowbias32(lowbias32(update * 0x85EBCA6BU + hi) ^ lo ^ 0x27D4EB2FU);
}

// ---- resources.hip ----
void launch_resources_begin(const DevWorld& W, hipStream_t s);
void launch_resources_end(const DevWorld& W, hipStream_t s);
void launch_resources_pack(const DevWorld& W, hipStream_t s);
bool res_stepped(const DevWorld& W);   // launch_resources_begin wrote res_amount_alt
void launch_resources_settle(const DevWorld& W, hipStream_t s, const unsigned long long* sum);

// ---- activate.hip: the placed births into their cells, the halo records ----
// fused: ACT_WORLD / ACT_STRIP; key, sub, nsub: the batch step's scheduler key and share
void launch_activate(const DevWorld& W, hipStream_t s, int fused, uint32_t key, int sub, int nsub);
void launch_halo_pack(const DevWorld& W, hipStream_t s);
void launch_activate_remote(const DevWorld& W, hipStream_t s, uint32_t key, int sub, int nsub);

// ---- stats.hip ----
// the update's statistics into d_stats (k_stats_partial + k_stats_final)
void launch_stats(const DevWorld& W, hipStream_t s, double* d_stats);

// ---- place.hip: placement, and the order of a step after interpretation ----
// placement and activation of batch step `sub` of `nsub` (key: its scheduler
// key), the newborns listed for the newborn pass; then launch_world_end
// pred_out (coherent mapped host memory, the update's last step): the
// predictor, its organisms and divide count, then pred_seq at system scope
void launch_world_post(const DevWorld& W, hipStream_t s, uint32_t key, int sub, int nsub,
                       long long* pred_out = nullptr, long long pred_seq = 0);
void launch_world_end(const DevWorld& W, hipStream_t s, double* d_stats, bool eager);
void launch_serial_post(const DevWorld& W, hipStream_t s, double* stats);
// strip tiles
void launch_tile_after_interpret(const DevWorld& W, hipStream_t s);
void launch_tile_place(const DevWorld& W, hipStream_t s, int round, int phase, uint32_t key, int sub, int nsub);
void launch_tile_finish(const DevWorld& W, hipStream_t s, uint32_t key, int sub, int nsub);

// the genotype table (genotypes.hip).  GtAgg: what a run of
// sorted positions of one genome key adds up to; GtScratch: the world's
// scratch for the grouping, allocated at the first avgpu_get_genotypes.
struct GtAgg {
  int32_t n, ng;            // members, members with a completed gestation
  double sm, sf, sr, mx;    // merit, fitness, 1 / gestation sums; max fitness (gestated members)
  int64_t sg, sc;           // gestation time, copied size sums (gestated members)
  int32_t first, pad;       // lowest cell
};
static_assert(sizeof(GtAgg) == 64, "GtAgg");
static_assert(sizeof(avgpu_genotype) == 80 && sizeof(avgpu_genotype_totals) == 32, "genotype table rows");
#define GT_SORT_TILE 4096   // (key, cell) pairs per radix sort block
#define GT_SEG_TILE 256     // sorted positions per segment tile
struct GtScratch {
  int64_t n, nblk, ntile;   // cells, sort tiles, segment tiles
  uint64_t* key[2];         // [n] key - 1 (ping-pong)
  int32_t* cell[2];         // [n]
  uint32_t* hist;           // [256][nblk]
  uint32_t* dtot;           // [256]
  GtAgg* tile_agg;          // [ntile] the tile's open tail part
  GtAgg* carry;             // [ntile] the open segment's parts before the tile
  int32_t* tile_flag;       // [ntile] a segment starts in the tile
  int32_t* tile_tails;      // [ntile] segments ending in the tile
  int64_t* row_off;         // [ntile] segments ending before the tile
  avgpu_genotype_totals* totals;
};
void launch_genotype_group(const DevWorld& W, const GtScratch& S, hipStream_t s);
void launch_genotype_rows(const DevWorld& W, const GtScratch& S, avgpu_genotype* d_out, hipStream_t s);
// the stable LSD radix sort of the grouping over S.key[0][0 .. m), m <= S.n:
// `passes` (even) 8-bit digits from bit 0; on completion S.key[0] holds the
// keys ascending and S.cell[0][r] the position key r came from
void launch_genotype_sort(const GtScratch& S, int64_t m, int passes, hipStream_t s);
// the device-resident genotype arbiter (arbiter.hip).
// ArbState: the world-level state; ArbWork: one classification's counters;
// ArbScratch: the world's buffers, allocated at the first
// avgpu_classify_genotypes / avgpu_set_arbiter -- 192 B per row of capacity
// (two state rows of 48 B, two keys of 8 B, the table row of 80 B).
static_assert(sizeof(avgpu_arbiter_row) == 48 && sizeof(avgpu_arbiter_summary) == 232, "arbiter rows");
struct ArbState {
  int64_t next_id, tot_genotypes, tot_threshold;
  uint64_t best_key;        // the previous dominant (0: none)
};
struct ArbWork {
  int32_t top, pad;         // the largest num_units
  unsigned long long best_id;   // the lowest id among the rows at the top
  unsigned long long num_new, num_matched, num_crossed, num_thr;
  int64_t stay_row;         // the previous dominant's row where it stays, else -1
  int64_t dom_row;
};
struct ArbScratch {
  int64_t cap;              // rows of capacity
  int cur;                  // which of row[] / key[] holds the state
  avgpu_arbiter_row* row[2];    // [cap] (swapped per classification)
  uint64_t* key[2];         // [cap] the rows' keys, dense (the match's binary search)
  avgpu_genotype* table;    // [cap] the table rows of the last classification
  ArbState* state;
  ArbWork* work;
  int64_t* sz_count;        // [AVGPU_MAX_GENOME + 1] names handed out per genome size
  avgpu_arbiter_summary* h_sum;   // pinned, host-mapped
  avgpu_arbiter_summary* d_sum;   // its device address
};
// the first part: after launch_genotype_group, the totals into the summary
void launch_arbiter_begin(const ArbScratch& A, const GtScratch& S, int64_t update, hipStream_t s);
// the rest: d_tab = the m table rows (launch_genotype_rows), n_prev the rows
// of state in A.row[A.cur]; the new state goes to A.row[A.cur ^ 1].  id_bits:
// every id of the new state is below 2^id_bits (<= 50).
void launch_arbiter_classify(const ArbScratch& A, const GtScratch& S, const avgpu_genotype* d_tab, int64_t m,
                             int64_t n_prev, int64_t update, int32_t threshold, int id_bits, hipStream_t s);
// the lineage store beside the arbiter (lineage.hip): the view
// a launch takes by value, assigned where a buffer is (re)allocated
static_assert(sizeof(avgpu_lineage_row) == 64 && sizeof(avgpu_lineage_summary) == 64, "lineage rows");
enum { LIN_ORPHANS = 0, LIN_UNSEQ = 1, LIN_TOTAL_A = 2, LIN_TOTAL_B = 3, LIN_MAXDEPTH = 4, LIN_CTR_WORDS = 8 };
struct LinScratch {
  avgpu_lineage_row* rows;  // [cap] ascending by id
  int64_t n, cap;
  uint8_t* arena;           // [arena_cap] captured birth genomes, 16-B aligned offsets in id order
  int64_t arena_bytes, arena_cap;
  unsigned long long* ctr;  // [LIN_CTR_WORDS] (LIN_* above; the first two cumulative)
  int64_t* idx;             // [scap] scratch: sizes / positions (scans)
  int64_t* asz;             // [scap] scratch: arena sizes of a prune
  uint32_t* mark;           // [scap] a prune's mark words
  int32_t* newcell;         // [scap] first cell of each new row of a classification
  int64_t scap;
};
// one classification's store maintenance, after launch_arbiter_classify and
// the swap of A.cur: n_prev rows before, m after, ids id0 .. id0 + n_new - 1
// new; leaves the arena total in ctr[LIN_TOTAL_A] for the host to reserve,
// then launch_lineage_copy captures the genomes
void launch_lineage_classify(const LinScratch& L, const ArbScratch& A, const DevWorld& W, int64_t n_prev, int64_t m,
                             int64_t id0, int64_t n_new, int64_t update, hipStream_t s);
void launch_lineage_copy(const LinScratch& L, const DevWorld& W, int64_t n_new, hipStream_t s);
// a prune: marks, positions (ctr[LIN_TOTAL_A] rows kept, ctr[LIN_TOTAL_B] arena bytes kept), then the compaction
void launch_lineage_mark(const LinScratch& L, hipStream_t s);
void launch_lineage_compact(const LinScratch& L, avgpu_lineage_row* out, int64_t out_cap, uint8_t* out_arena,
                            int64_t out_arena_cap, hipStream_t s);
void launch_lineage_max_depth(const LinScratch& L, hipStream_t s);
// mutational landscapes (landscape.hip).  The mutants of every
// base genome are numbered back to back: mutant m of the call is rank
// m - mut_off[g] of genome g.  Ranks are cut into tiles of LAND_TILE aligned
// to each genome's rank 0 (a genome's last tile may be short); a chunk of the
// scratch test world holds whole tiles, packed densely across genomes.
#define LAND_TILE 256
// how a rank becomes a mutant: the base genome itself, one or two
// substitutions (cLandscape::Process_Body), one insertion (ProcessInsert),
// one deletion (ProcessDelete)
enum { LAND_BASE = 0, LAND_SUB1 = 1, LAND_SUB2 = 2, LAND_INS = 3, LAND_DEL = 4 };
// what a tile of ranks, or a genome's tiles, add up to
struct LandPart {
  double sf, sq, sp, sn;    // sums of fitness, its square, beneficial and deleterious fitness
  double pf;                // peak: the largest beneficial fitness (-1: none) ...
  int64_t pr;               // ... and the lowest rank attaining it
  int32_t dead, neg, neut, pos;
  int32_t run1, run2;       // mutants run at recursion depth 1, 2
  int64_t pad;
};
static_assert(sizeof(LandPart) == 80, "LandPart");
// ... and what a tile of pair mutants adds up to (cLandscape::TestMutPair)
struct LandEpiPart {
  double sn, sp, s0;        // sums of combo fitness: antagonistic, synergistic, no epistasis
  int64_t dead, neg, pos, none;
  int64_t run1, run2;       // pair mutants run at recursion depth 1, 2
};
static_assert(sizeof(LandEpiPart) == 72, "LandEpiPart");
struct LandScratch {
  int64_t chunk;            // cells of the scratch test world
  // the call's inputs (uploaded per call)
  int32_t n, num_insts, time_mod, pad0;
  const uint8_t* base_op;   // base genomes in op codes, genome g at base_off[g] (16-B aligned, zero padded,
                            // one zero group behind the last genome)
  const uint8_t* base_code; // the same in canonical codes
  const int64_t* base_off;  // [n]
  const int32_t* len;       // [n]
  const int64_t* mut_off;   // [n + 1] mutants before genome g
  const int64_t* tile_off;  // [n + 1] tiles before genome g
  const int64_t* site_off;  // [n] sites before genome g (site_count / chart rows; an insertion
                            // landscape has len + 1 of them per genome)
  const uint8_t* op2code;   // [AVGPU_MAX_INST]
  // per genome
  double* base_fit;         // [n] ProcessBase: colony fitness,
  double* base_merit;       // colony organism's merit,
  int32_t* base_gest;       // its gestation time
  LandPart* parts;          // [tiles]
  avgpu_landscape* rows;    // [n]
  int32_t* site_count;      // [sites] or NULL
  double* chart;            // [sites][num_insts] or NULL
  LandEpiPart* eparts;      // [tiles] of the pair mutants (avgpu_landscape_pairs)
  avgpu_epistasis* erows;   // [n]
  // per chunk (kept with the scratch world)
  int32_t* budget;          // [chunk] budget row of the depth being run
  double* fit;              // [chunk] colony fitness of the chunk's mutant i
  uint8_t* dep;             // [chunk] the depth its verdict fell at
  int32_t* src[2];          // [chunk] depth d + 1's cell j runs the offspring of depth d's cell src[d][j]
  uint8_t* gen[2];          // [chunk][TAPE_SLOT] the genome depth d + 1's cell j runs
  int32_t* glen[2];         // [chunk] its length
  int32_t* count;           // [2] survivors listed for depth 1, 2
};
// cells [0, cnt) take the chunk's mutants m0 .. m0 + cnt - 1 (mode LAND_*; LAND_BASE: the base genomes themselves)
void launch_land_seed(const DevWorld& W, const LandScratch& S, hipStream_t s, int mode, int64_t m0, int cnt);
// cells [0, cnt) take the offspring listed for depth 1 or 2
void launch_land_seed_next(const DevWorld& W, const LandScratch& S, hipStream_t s, int depth, int cnt);
void launch_land_judge(const DevWorld& W, const LandScratch& S, hipStream_t s, int mode, int depth, int64_t m0,
                       int cnt);
// tiles [t0, t1) of the chunk that starts at mutant m0
void launch_land_reduce(const LandScratch& S, hipStream_t s, int mode, int64_t m0, int64_t t0, int64_t t1);
// distance: the value the rows report (cLandscape's `distance` member)
void launch_land_rows(const LandScratch& S, hipStream_t s, int distance);
// the pair mutants' tiles [t0, t1) against S.chart, and their rows
void launch_land_epi_reduce(const LandScratch& S, hipStream_t s, int64_t m0, int64_t t0, int64_t t1);
void launch_land_epi_rows(const LandScratch& S, hipStream_t s);
// genetic distances and the consensus histogram (distance.hip):
// the world's scratch, grown by 1.25x with the largest call seen
struct DistScratch {
  uint8_t* gen;             // the call's genomes, each at a 16-B aligned offset, zero padded to 16 B
                            // (avgpu_cell_distances: the reference genome in canonical codes)
  int64_t* off;             // [n] their offsets
  int32_t* len;             // [n]
  int32_t* pair_a;          // [npairs] indices into the n genomes
  int32_t* pair_b;
  int32_t* ham;             // [npairs] or [count]
  int32_t* edit;
  int32_t* hist;            // [TAPE_SLOT][AVGPU_MAX_INST + 1] by handler, column 0 "no site"
  unsigned long long* living;   // the living cells k_site_hist counted
};
static_assert(AVGPU_MAX_GENOME == TAPE_SLOT, "a site histogram row per tape site (MAX_GENOME_LENGTH)");
// one wave per pair / per cell; a NULL-ed output (want_* false) is not computed
void launch_pair_dist(const DistScratch& S, hipStream_t s, int npairs, bool want_ham, bool want_edit);
void launch_cell_dist(const DevWorld& W, const DistScratch& S, hipStream_t s, int64_t first, int64_t count,
                      int ref_len, bool want_ham, bool want_edit);
// S.hist and S.living zeroed by the caller
void launch_site_hist(const DevWorld& W, const DistScratch& S, hipStream_t s, int64_t first, int64_t count);
// population events (popevents.hip): kills decided on the device.
// A killed cell loses CTL_ALIVE and nothing else (avgpu_kill).  EvScratch: the
// world's scratch, one allocation; the caller zeroes killed, sel and hist
// (EV_ZERO_BYTES from killed) before a launch.
#define EV_DIGIT_BITS 8                     // the select's digit: four passes over a 32-bit word
#define EV_BINS (1 << EV_DIGIT_BITS)
#define EV_PASSES (32 / EV_DIGIT_BITS)
struct EvSelect {
  uint32_t prefix;          // the digits of the threshold chosen so far (high bits)
  uint32_t kill_all;        // keep == 0
  uint64_t rank;            // the rank still looked for among the words with that prefix, 1-based;
                            // 0: no threshold (keep >= living), nobody dies
};
struct EvScratch {
  unsigned long long* killed;   // the living organisms the call killed
  EvSelect* sel;
  uint32_t* hist;           // [EV_PASSES][EV_BINS] the select's digit counts
  const int64_t* cells;     // [n] avgpu_kill_cells' ids
  const uint64_t* keys;     // [nkeys] avgpu_kill_genotypes' keys, ascending, distinct
};
#define EV_ZERO_BYTES (16 + sizeof(EvSelect) + sizeof(uint32_t) * EV_PASSES * EV_BINS)
void launch_kill_cells(const DevWorld& W, const EvScratch& S, hipStream_t s, int64_t n);
// every living cell with event_draw(base, cell) < th dies; nkeys >= 0: only those whose gkey is among S.keys
void launch_kill_prob(const DevWorld& W, const EvScratch& S, hipStream_t s, uint32_t base, uint64_t th, int64_t nkeys);
// rows y1 .. y2, columns x1 .. x2 of the torus, as cActionKillRectangle's loops walk them (0 <= x1 <= x2 < x1 + X)
void launch_kill_rect(const DevWorld& W, const EvScratch& S, hipStream_t s, int x1, int y1, int x2, int y2);
// the living cells with the `keep` smallest words survive
void launch_keep_sample(const DevWorld& W, const EvScratch& S, hipStream_t s, uint32_t base, int64_t keep);
