/*
 * dslabs_hip.h -- C ABI of libdslabs_hip.so, the MI355X breadth-first model-checking engine.
 *
 * This ABI is the drop-in boundary for the reference's BFS strategy. The reference has no
 * FFI (it is pure Java); each entry point below replaces a piece of the Java search and is what a
 * `GpuBFS extends Search` strategy binds through JNI / Panama FFM.
 * Paths are relative to the reference root, T = framework/tst/dslabs/framework/testing.
 *
 *   dsl_create          <- `new BFS(settings)` + the NodeGenerator / addServer / addClientWorker
 *                          calls that build the initial SearchState
 *                          (T/search/Search.java:390-395, T/AbstractState.java:207-241)
 *   dsl_set_settings    <- SearchSettings / TestSettings: maxDepth, maxTimeSecs, invariants,
 *                          goals, prunes, link/sender/receiver filters, timer masks
 *                          (T/search/SearchSettings.java:43-135, T/TestSettings.java:46-245)
 *   dsl_set_initial     <- starting a search from a non-initial SearchState (a goal state of an
 *                          earlier search, depth > 0), e.g. PaxosTest.java:898-910
 *   dsl_run             <- Search.run(initialState) for BFS (T/search/Search.java:233-388,
 *                          :405-505): returns the SearchResults equivalent
 *   dsl_result_free     <- (GC in Java)
 *   dsl_progress        <- BFS.status() "Explored: N, Depth: D" (T/search/Search.java:426-431)
 *   dsl_last_error      <- Java exceptions on infrastructure errors
 *
 * Conventions: every function returning int returns DSL_OK (0) or a negative dsl_status.
 * Caller-owned input buffers are copied during the call. dsl_result is library-allocated and
 * released with dsl_result_free. One engine per calling thread; dsl_run blocks.
 */
#ifndef DSLABS_HIP_H_
#define DSLABS_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSL_ABI_VERSION 6 /* 2: dsl_set_dropped; dsl_stats host_syncs / table_rehashes / rccl_version;
                            3: dsl_engine_config.flags, dsl_host_comm.flags;
                            4: dsl_settings.do_checks / check_sample, dsl_result check counts,
                               dsl_stats exchange_rounds / fast_levels / completions;
                            5: dsl_stats deduped;
                            6: dsl_settings.max_terminals, dsl_result terminals_total / n_terminals /
                               terminals, dsl_terminal.
                            Still 6 with DSL_PRED_FIELD and DSL_PRED_NET / _REC_COND: a new dsl_predicate_id
                            changes no struct and adds no entry point; a library without it answers
                            DSL_ERR_UNKNOWN_PREDICATE.
                            Still 6 with dsl_set_watches / dsl_watch_counts: two entry points are
                            added, no struct changes; a caller that never names them runs as before.
                            Still 6 with dsl_set_watch_witnesses / dsl_watch_witness: the same again
                            Still 6 with dsl_set_event_census / dsl_event_census / dsl_event_class_count /
                            _name / _is_timer: five entry points and dsl_event_count are added;
                            dsl_settings, dsl_result and dsl_stats keep their bytes
                            Still 6 with dsl_set_step_invariants / dsl_step_edges / dsl_step_violation and
                            the DSL_PRED_STEP_* leaves: three entry points, no struct changes */
#define DSL_MAX_NODES 32
#define DSL_MAX_PREDICATES 16
#define DSL_MAX_POOL 48          /* operands of combinator predicates (dsl_settings.pool) */
#define DSL_MAX_PARAMS 64
#define DSL_MAX_EVENT_FIELDS 8

typedef enum {
  DSL_OK = 0,
  DSL_ERR_ARG = -1,
  DSL_ERR_HIP = -2,
  DSL_ERR_TABLE_FULL = -3,        /* visited table capacity exhausted */
  DSL_ERR_FRONTIER_FULL = -4,     /* next frontier exceeds its capacity */
  DSL_ERR_STATE_OVERFLOW = -5,    /* a successor exceeded the packed state's bounded message
                                     set / timer list / log (never silently truncated) */
  DSL_ERR_UNKNOWN_PROTOCOL = -6,
  DSL_ERR_UNKNOWN_PREDICATE = -7,
  DSL_ERR_COMM = -8,
  DSL_ERR_NO_DEVICE = -9
} dsl_status;

/* SearchResults.EndCondition (T/search/SearchResults.java:35-41), same order of priority. */
typedef enum {
  DSL_EXCEPTION_THROWN = 0,
  DSL_INVARIANT_VIOLATED = 1,
  DSL_GOAL_FOUND = 2,
  DSL_SPACE_EXHAUSTED = 3,
  DSL_TIME_EXHAUSTED = 4
} dsl_end_condition;

/* Protocols with device transition functions. */
typedef enum {
  DSL_PROTO_PINGPONG = 1,   /* lab0 PingPong (labs/lab0-pingpong/src/dslabs/pingpong) */
  DSL_PROTO_SIPAXOS = 2,    /* single-instance Paxos (T/visualization/examples/paxosmadesimple) */
  DSL_PROTO_SYNTHETIC = 3,  /* table-driven synthetic protocol (BASELINE config C3) */
  DSL_PROTO_AMOKV = 4,      /* lab1 at-most-once KV client/server (BASELINE config C2) */
  DSL_PROTO_MULTIPAXOS = 5, /* lab3 Multi-Paxos (BASELINE config C5) */
  DSL_PROTO_PB = 6,         /* lab2 primary-backup + ViewServer (BASELINE config C4) */
  DSL_PROTO_MINITEST = 7,   /* the two-node fixture of SearchAndTraceMinimizerTest (tst-self) */
  DSL_PROTO_PINGPONG_IR = 8, /* lab0 PingPong generated from the protocol IR (dslabs_amd/ir/specs/pingpong.py) */
  DSL_PROTO_AMOKV_IR = 9,    /* lab1 AMO KV generated from the protocol IR (dslabs_amd/ir/specs/amokv.py) */
  DSL_PROTO_MULTIPAXOS_IR = 10, /* lab3 Multi-Paxos (C5) generated from the protocol IR (dslabs_amd/ir/specs/multipaxos.py) */
  DSL_PROTO_PB_IR = 11          /* lab2 primary-backup + ViewServer (C4) generated from the protocol IR (dslabs_amd/ir/specs/pb.py) */
} dsl_protocol_id;

typedef struct {
  int32_t protocol;              /* dsl_protocol_id */
  int32_t n_params;
  int64_t params[DSL_MAX_PARAMS];/* protocol parameters, see dslabs_amd/protocols.py */
} dsl_protocol_desc;

/* Standard predicates (T/StatePredicate.java:52-83) and protocol predicates.
 * Args are node indices / counts as documented per predicate. */
typedef enum {
  DSL_PRED_RESULTS_OK = 1,          /* "Clients got expected results" */
  DSL_PRED_CLIENTS_DONE = 2,        /* "All clients' workloads finished" */
  DSL_PRED_CLIENT_DONE = 3,         /* clientDone(addr): arg0 = node index */
  DSL_PRED_NONE_DECIDED = 4,        /* "No results returned" */
  DSL_PRED_CLIENT_HAS_RESULTS = 5,  /* clientHasResults(addr, n): arg0 node, arg1 n */
  DSL_PRED_SIP_AGREEMENT = 100,     /* SingleInstancePaxos "Agreement" */
  DSL_PRED_SIP_INTEGRITY = 101,     /* SingleInstancePaxos "Integrity" */
  DSL_PRED_SIP_TERMINATION = 102,   /* SingleInstancePaxos "Termination" */
  DSL_PRED_SYNTH_NOT_ALL_MAX = 200, /* synthetic: not every node word at its maximum */
  DSL_PRED_SYNTH_COUNTER_LT = 201,  /* synthetic: node word arg0 < arg1 */
  DSL_PRED_APPENDS_LINEARIZABLE = 300, /* KVStoreWorkload.APPENDS_LINEARIZABLE */
  DSL_PRED_LOGS_CONSISTENT = 400,   /* PaxosTest LOGS_CONSISTENT_ALL_SLOTS (PaxosTest.java:302-322) */
  DSL_PRED_LOGS_CONSISTENT_ACTIVE = 401, /* PaxosTest LOGS_CONSISTENT (:282-300) */
  DSL_PRED_SLOT_VALID = 402,        /* PaxosTest slotValid(i) (:276-279): arg0 = slot */
  DSL_PRED_HAS_STATUS = 403,        /* PaxosTest hasStatus(a, i, s) (:113-117): arg0 = server node,
                                       arg1 = slot << 4 | PaxosLogSlotStatus ordinal */
  DSL_PRED_HAS_COMMAND = 404,       /* PaxosTest hasCommand(a, i, c) (:119-123): arg0 = server node,
                                       arg1 = slot << 8 | KV command code (op << 2 | value; 0 = null) */
  DSL_PRED_PB_HAS_VIEW_REPLY = 500, /* PrimaryBackupTest.hasViewReply(n): arg0 = n */
  DSL_PRED_PB_VIEW_REPLY_EXACT = 501,  /* hasViewReply(n, p, b) (:112-117): arg0 = view (num | p << 4 | b << 6) */
  DSL_PRED_PB_VIEW_REPLIES_SENT = 502, /* initView's "ViewReply for v sent to nodes ..., primary ack sent"
                                          (PrimaryBackupTest.java:136-156): arg0 = view, arg1 = mask of
                                          recipient node indices */
  DSL_PRED_MINI_FOO = 700,          /* SearchAndTraceMinimizerTest foo: !a.foo */
  DSL_PRED_MINI_FOO_EXCEPTION = 701,    /* fooException: throws when a.foo, else true */
  DSL_PRED_MINI_ALWAYS_EXCEPTION = 702, /* alwaysException: always throws */
  /* Combinators (T/StatePredicate.java:397-431): arg0 / arg1 index the operands in
   * dsl_settings.pool (an operand may itself be a combinator of lower pool entries). With the
   * reference's short-circuit semantics: a throwing left operand throws; and(a, b) is a when a
   * is false, else b; or(a, b) is a when a is true, else b; implies(a, b) = or(negate(a), b). */
  DSL_PRED_AND = 900,
  DSL_PRED_OR = 901,
  DSL_PRED_IMPLIES = 902,
  /* The generic field leaf (StatePredicate.statePredicate(name, fn), T/StatePredicate.java:168-176,
   * for fn = a comparison over node fields): an unsigned comparison of a bit field of one node's
   * words with a constant or with a second bit field. Every protocol accepts it; it never throws;
   * negate applies as for any leaf and it may be an operand of the combinators. Encoding below
   * (DSL_FIELD_*). A bad descriptor is refused by dsl_set_settings with DSL_ERR_ARG. */
  DSL_PRED_FIELD = 950,
  /* The generic network leaf (StatePredicate.containsMessageMatching(name, fn),
   * T/StatePredicate.java:139-149, for fn = a conjunction of comparisons of record fields with
   * constants): true when network() -- the state's records and the dropped records,
   * SearchState.java:153-157 -- holds a record that satisfies ALL of the leaf's conditions.
   * arg0 = index of the first condition in dsl_settings.pool, arg1 = number of conditions
   * (1 .. DSL_MAX_NET_CONDS); the conditions are consecutive DSL_PRED_REC_COND pool entries. Every
   * protocol accepts it; it never throws; negate applies as for any leaf and it may be an operand
   * of the combinators. A bad leaf is refused by dsl_set_settings with DSL_ERR_ARG. */
  DSL_PRED_NET = 951,
  /* One condition of a DSL_PRED_NET: an unsigned comparison of a bit field of the record with a
   * constant. Legal only as a pool entry that a DSL_PRED_NET refers to (never a predicate, never a
   * combinator's operand); negate must be 0. Encoding below (DSL_REC_*). */
  DSL_PRED_REC_COND = 952,
  /* The step leaves: legal only inside a step invariant (dsl_set_step_invariants below), where a
   * predicate is judged on an edge (parent P, event E, successor X). Anywhere else -- invariants,
   * goals, prunes, watches -- they are refused with DSL_ERR_ARG.
   * DSL_PRED_STEP_FIELD: DSL_PRED_FIELD's encoding plus two bits of arg0: bit 36 = the left operand
   * is read from X (otherwise from P), bit 37 = the same for a right operand that is a field.
   * Unsigned comparison, never throws, any two nodes; descriptors are checked as DSL_PRED_FIELD's. */
  DSL_PRED_STEP_FIELD = 953,
  /* DSL_PRED_STEP_SENT: the step added to the network a record satisfying all of the leaf's
   * conditions; DSL_PRED_NET's pool encoding (arg0 = first DSL_PRED_REC_COND entry, arg1 = their
   * number), counted against DSL_MAX_NET_CONDS_TOTAL. "Added" means new to P's record set: the
   * network is a set, so a record the handler sends again while P already holds it is NOT added
   * and does not match. */
  DSL_PRED_STEP_SENT = 954,
  /* DSL_PRED_STEP_EVENT: E is of handler class arg0 (an index of dsl_event_class_name's range, -1 =
   * any) and is delivered to node arg1 (-1 = any; a timer's node is its own). An event the engine
   * would skip as a proven no-op is judged under its real class, as the event census counts it. */
  DSL_PRED_STEP_EVENT = 955
} dsl_predicate_id;

#define DSL_STEP_LHS_NEW_BIT 36
#define DSL_STEP_RHS_NEW_BIT 37
#define DSL_STEP_FIELD_ARG0(desc, cmp, rhs_is_field, lhs_new, rhs_new)                    \
  (DSL_FIELD_ARG0(desc, cmp, rhs_is_field) | ((int64_t)((lhs_new) ? 1 : 0) << DSL_STEP_LHS_NEW_BIT) | \
   ((int64_t)((rhs_new) ? 1 : 0) << DSL_STEP_RHS_NEW_BIT))
#define DSL_STEP_ARG0_LHS_NEW(arg0) ((int)(((uint64_t)(arg0) >> DSL_STEP_LHS_NEW_BIT) & 1u))
#define DSL_STEP_ARG0_RHS_NEW(arg0) ((int)(((uint64_t)(arg0) >> DSL_STEP_RHS_NEW_BIT) & 1u))

/* DSL_PRED_FIELD. A field descriptor (27 bits) names `width` bits (1..32) from bit `bit` of node
 * `node`'s words (bit 0 = the least significant bit of the node's word 0; the field lies inside
 * one 32-bit word: (bit % 32) + width <= 32, and inside the node: bit + width <= 32 * the
 * protocol's words per node):
 *     descriptor = bit (bits 0-15) | width << 16 (bits 16-21) | node << 22 (bits 22-26)
 * dsl_predicate.arg0 = left descriptor (bits 0-31) | comparison << 32 (bits 32-34)
 *                      | (right operand is a field) << 35; every other bit 0
 * dsl_predicate.arg1 = an unsigned constant 0 .. 2^32-1, or the right operand's descriptor
 * The predicate is  left <comparison> right  over the unsigned field values. */
#define DSL_CMP_EQ 0
#define DSL_CMP_NE 1
#define DSL_CMP_LT 2
#define DSL_CMP_GE 3
#define DSL_CMP_LE 4
#define DSL_CMP_GT 5
#define DSL_FIELD_DESC(node, bit, width) \
  (((uint32_t)(node) << 22) | ((uint32_t)(width) << 16) | (uint32_t)(bit))
#define DSL_FIELD_BIT(desc) ((int)((uint32_t)(desc) & 0xffffu))
#define DSL_FIELD_WIDTH(desc) ((int)(((uint32_t)(desc) >> 16) & 0x3fu))
#define DSL_FIELD_NODE(desc) ((int)(((uint32_t)(desc) >> 22) & 0x1fu))
#define DSL_FIELD_DESC_MASK 0x07ffffffu
#define DSL_FIELD_ARG0(desc, cmp, rhs_is_field) \
  ((int64_t)(uint32_t)(desc) | ((int64_t)(cmp) << 32) | ((int64_t)((rhs_is_field) ? 1 : 0) << 35))
#define DSL_FIELD_ARG0_DESC(arg0) ((uint32_t)((uint64_t)(arg0) & 0xffffffffu))
#define DSL_FIELD_ARG0_CMP(arg0) ((int)(((uint64_t)(arg0) >> 32) & 7u))
#define DSL_FIELD_ARG0_RHS_IS_FIELD(arg0) ((int)(((uint64_t)(arg0) >> 35) & 1u))

/* DSL_PRED_REC_COND. `width` bits (1..32) from bit `bit` of the protocol's packed record (bit 0 =
 * the record's least significant bit; bit + width <= 8 * the record's size in bytes; on a 64-bit
 * record the field may cross bit 32, the record is shifted as one value):
 *     dsl_predicate.arg0 = bit (bits 0-15) | width << 16 (bits 16-21) | comparison << 32 (bits 32-34);
 *                          every other bit 0
 *     dsl_predicate.arg1 = an unsigned constant 0 .. 2^32-1
 * The condition is  field <comparison> constant  (DSL_CMP_*) over the unsigned field value. */
#define DSL_MAX_NET_CONDS 8       /* conditions of one DSL_PRED_NET */
#define DSL_MAX_NET_CONDS_TOTAL 32 /* conditions of all the network leaves of one dsl_settings */
#define DSL_REC_ARG0(bit, width, cmp) \
  ((int64_t)(uint32_t)(bit) | ((int64_t)(uint32_t)(width) << 16) | ((int64_t)(cmp) << 32))
#define DSL_REC_ARG0_BIT(arg0) ((int)((uint64_t)(arg0) & 0xffffu))
#define DSL_REC_ARG0_WIDTH(arg0) ((int)(((uint64_t)(arg0) >> 16) & 0x3fu))
#define DSL_REC_ARG0_CMP(arg0) ((int)(((uint64_t)(arg0) >> 32) & 7u))
#define DSL_REC_ARG0_MASK 0x00000007003fffffull

typedef struct {
  int32_t pred_id;   /* dsl_predicate_id */
  int32_t negate;    /* StatePredicate.negate() */
  int64_t arg0, arg1;
} dsl_predicate;

#define DSL_TRISTATE_UNSET (-1)

typedef struct {
  int32_t max_depth;        /* SearchSettings.maxDepth, -1 = unlimited (absolute depth) */
  int32_t max_time_ms;      /* TestSettings.maxTimeSecs*1000, -1 = unlimited; checked per level */
  int32_t network_active;   /* TestSettings.networkActive */
  int32_t deliver_timers;   /* TestSettings.deliverTimers (global default) */
  int8_t link_active[DSL_MAX_NODES][DSL_MAX_NODES]; /* [from][to]: -1 unset, 0, 1 */
  int8_t sender_active[DSL_MAX_NODES];
  int8_t receiver_active[DSL_MAX_NODES];
  int8_t timers_active[DSL_MAX_NODES];
  int32_t n_invariants, n_goals, n_prunes;          /* ordered, as inserted */
  dsl_predicate invariants[DSL_MAX_PREDICATES];
  dsl_predicate goals[DSL_MAX_PREDICATES];
  dsl_predicate prunes[DSL_MAX_PREDICATES];
  /* engine capacity knobs (0 = automatic) */
  int32_t table_log2_slots; /* first visited table = 2^k 8-byte slots per shard (0: 2^20); it grows
                               at level boundaries, kept at most half full */
  int32_t n_pool;           /* entries of pool[] */
  uint64_t max_frontier_states; /* a level whose frontier holds more states ends the search with
                                   DSL_ERR_FRONTIER_FULL (0: no cap) */
  uint64_t memory_budget_bytes; /* device memory the visited table may grow to, per shard (0: no cap;
                                   a search that needs more ends with DSL_ERR_TABLE_FULL) */
  dsl_predicate pool[DSL_MAX_POOL]; /* operands of DSL_PRED_AND / _OR / _IMPLIES predicates */
  /* GlobalSettings.doErrorChecks / doAllChecks (T/search/Search.java:201-220): after every level,
     up to check_sample of its new VALID states (0: 256) are re-derived on the host from their
     parent and event (stepEvent, SearchState.java:282-359) and compared with the device's row
     (determinism); with DSL_CHECKS_ALL a delivered message is also stepped a second time on the
     successor (idempotence, not necessarily an error). Counts in dsl_result. */
  int32_t do_checks;        /* DSL_CHECKS_* */
  int32_t check_sample;
  /* Every terminal state of the level that ends a BFS (dsl_result.terminals), at most this many
     listed; 0 = off: only the one reported terminal, as before ABI 6. Read by dsl_run alone. */
  int32_t max_terminals;
  int32_t reserved;
} dsl_settings;

/* dsl_settings.do_checks */
#define DSL_CHECKS_NONE 0
#define DSL_CHECKS_ERRORS 1 /* GlobalSettings.doErrorChecks: determinism */
#define DSL_CHECKS_ALL 2    /* GlobalSettings.doAllChecks: + idempotence of message handlers */

typedef struct {
  int32_t device;           /* HIP device ordinal, -1 = current */
  int32_t rank, world_size; /* shard index / number of shards (one process or thread per GPU) */
  int32_t virtual_shards;   /* >1: emulate that many hash shards on this one device (tests) */
  uint8_t comm_id[128];     /* RCCL ncclUniqueId when world_size > 1 */
  int64_t replicate_below;  /* multi-shard: a level whose frontier is smaller runs replicated on every
                               shard (no exchange); -1 = automatic (a per-level cost decision),
                               0 = always hash-sharded, n > 0 = below n states */
  int32_t flags;            /* DSL_CFG_* */
  int32_t reserved;
} dsl_engine_config;

/* dsl_engine_config.flags */
#define DSL_CFG_RCCL_AT_WORLD_1 1 /* build the RCCL communicator (comm_id) also at world_size 1, so the
                                     collectives' code runs on a one-GPU box (tests) */

/* A decoded event (MessageEnvelope / TimerEnvelope, T/MessageEnvelope.java, T/TimerEnvelope.java). */
typedef struct {
  int32_t is_timer;
  int32_t from, to;         /* node indices (from == to for timers) */
  int32_t type;             /* protocol message / timer type id */
  int32_t n_fields;
  int32_t timer_min, timer_max;
  int32_t reserved;
  int64_t fields[DSL_MAX_EVENT_FIELDS];
} dsl_event;

/* One terminal state of the level that ended a BFS (dsl_result.terminals). */
typedef struct {
  int32_t end_condition;    /* DSL_EXCEPTION_THROWN, DSL_INVARIANT_VIOLATED or DSL_GOAL_FOUND */
  int32_t predicate_index;  /* index in invariants[] / goals[] that fired first, -1 for an exception */
  int32_t trace_len;        /* terminal_depth - initial_depth */
  int32_t reserved;
  dsl_event* trace;         /* [trace_len]: events from the initial state to this terminal */
  uint8_t* state;           /* packed state (dsl_result.state_bytes), the trace replayed on the host */
} dsl_terminal;

typedef struct {
  int32_t end_condition;    /* dsl_end_condition */
  int32_t terminal_depth;   /* depth of the reported terminal state, -1 if none */
  int32_t predicate_index;  /* index in invariants[] / goals[] that fired, -1 if none */
  int32_t max_depth;        /* deepest discovered state (BFS.depth) */
  uint64_t states;          /* unique states, reference counting rule (Search.java:470-490) */
  int32_t n_levels;
  int32_t trace_len;
  uint64_t* per_depth;      /* [n_levels]: states discovered at depth initial_depth + i */
  dsl_event* trace;         /* [trace_len]: events from the initial state to the terminal */
  uint8_t* terminal_state;  /* packed terminal state (state_bytes), NULL if none */
  uint32_t state_bytes;
  int32_t initial_depth;
  double elapsed_s;         /* wall time of the search (excludes dsl_create) */
  uint64_t successors;      /* successor states generated (events applied) */
  uint64_t new_states_inserted;
  uint64_t exchanged_states;/* states routed to another shard (multi-GPU) */
  double level_ms_max;
  /* dsl_settings.do_checks (CheckLogger.notDeterministic / notIdempotent, T/utils/CheckLogger.java:104-121):
     successors re-checked, and how many of them were not deterministic / not idempotent; the first
     offending event (its parent's depth and the event, decoded) of each kind */
  uint64_t checks_run;
  uint64_t not_deterministic;
  uint64_t not_idempotent;
  dsl_event first_not_deterministic;
  dsl_event first_not_idempotent;
  /* dsl_settings.max_terminals > 0 and a dsl_run that ended EXCEPTION_THROWN, INVARIANT_VIOLATED or
     GOAL_FOUND: every terminal of the level that ended the search. BFS finishes that level
     (Search.java:370-385 keeps the best of it by priority), and this is the whole set: every
     distinct state first discovered at terminal_depth that checkState judges TERMINAL
     (Search.java:468-504), listed once however many (parent, event) pairs reach it, and every
     exceptional successor generated at that level, one per (parent, event) and never merged (a
     Throwable equals only itself). A terminal initial state is the whole list.
     Order: ascending by priority (EXCEPTION, INVARIANT, GOAL), then by the state's 128-bit
     fingerprint, so terminals[0] is the terminal reported above (same state, end condition and
     predicate index) and the listed states never depend on arrival order or on sharding; a trace
     is A shortest trace (a state with two parents may be recorded through either).
     terminals_total is the whole count; the list holds the first min(terminals_total,
     max_terminals) of that order, and only those have a trace and a state.
     A level cut short by max_time_ms is not enumerated: the list is the reported terminal alone
     and terminals_total = 1. Any other result (and dsl_run_dfs, dsl_replay,
     dsl_human_readable_trace): terminals_total = 0, n_terminals = 0, terminals = NULL.
     A search over more than one process (world_size > 1) with max_terminals > 0 is refused with
     DSL_ERR_ARG; virtual shards in one process are supported. */
  uint64_t terminals_total;
  int32_t n_terminals;
  int32_t reserved;
  dsl_terminal* terminals;  /* [n_terminals] */
} dsl_result;

typedef struct dsl_engine dsl_engine;

int dsl_abi_version(void);
int dsl_device_count(void);
int dsl_state_bytes(const dsl_protocol_desc* proto);
/* The protocol's initial packed state (every node added and init()-ed, SearchState.addServer /
 * addClientWorker order), computed on the host: no engine or device needed. */
int dsl_init_state(const dsl_protocol_desc* proto, uint8_t* packed, size_t len);
/* SearchState.dropPendingMessages (T/search/SearchState.java:538-541) on a packed state: every
 * message of its network moves into the caller's dropped set (`dropped`: one record per uint64,
 * kept sorted and duplicate-free; *n_dropped is read and updated; DSL_ERR_ARG past `cap`). Events
 * only come from the remaining (undropped) network. The dropped set never changes during a search
 * that starts from such a state, so search-equivalence (SearchEquivalenceWrappedSearchState,
 * :575-619: equal union of both sets and equal undropped sets) is equality of the packed states
 * and the engine needs nothing more: the caller keeps the set with the state and its successors. */
int dsl_drop_pending_messages(const dsl_protocol_desc* proto, uint8_t* packed, size_t len, uint64_t* dropped,
                              int32_t cap, int32_t* n_dropped);
/* undropMessages / undropMessagesFrom / undropMessagesTo (:543-561): the dropped messages sent by
 * address index `from` and addressed to `to` (-1 = any) are added back to the packed state's
 * network; the dropped set itself is unchanged, as in the reference. */
int dsl_undrop_messages(const dsl_protocol_desc* proto, uint8_t* packed, size_t len, const uint64_t* dropped,
                        int32_t n_dropped, int32_t from, int32_t to);
/* The dropped network of the search's start state (the set dsl_drop_pending_messages keeps, one
 * record per uint64): network predicates read network() = the state's network + these records
 * (SearchState.network(), T/search/SearchState.java:153-157; StatePredicate.containsMessageMatching,
 * T/StatePredicate.java:146-149). Constant for the search (every successor inherits the set); it
 * never adds events. n_dropped = 0 clears it. Copied during the call. */
int dsl_set_dropped(dsl_engine* e, const uint64_t* dropped, int32_t n_dropped);
int dsl_comm_unique_id(uint8_t out[128]);
int dsl_create(const dsl_protocol_desc* proto, const dsl_engine_config* cfg, dsl_engine** out);
int dsl_set_settings(dsl_engine* e, const dsl_settings* s);
int dsl_set_initial(dsl_engine* e, const uint8_t* packed, size_t len, int32_t depth);
int dsl_get_initial(dsl_engine* e, uint8_t* packed, size_t len);
int dsl_run(dsl_engine* e, dsl_result** out);
int dsl_progress(dsl_engine* e, uint64_t* states, int32_t* depth);

/* Watches: predicates that are only counted. An invariant, a goal or a prune ends the search or
 * cuts it; a watch changes nothing (the same states, per_depth, end condition, terminals, traces
 * and check counts with or without it) and answers "was this situation reached in this search,
 * how early, how often" -- the coverage side of StatePredicate (T/StatePredicate.java), for which
 * the reference's tests run one extra goal search per scenario. Every state dsl_run counts in
 * per_depth is evaluated once against each watch, at the depth where it was first discovered
 * (BFS.exploreNode's discovered.add, Search.java:468-504): the start state at index 0, then every
 * newly inserted successor whatever its verdict -- valid, pruned, a goal or invariant terminal, a
 * maxDepth state. An exceptional successor has no state and is not evaluated. A watch counts when
 * it is true after its negation; a watch that throws counts as not holding. A watch is any
 * predicate the settings accept (a named leaf, DSL_PRED_FIELD, DSL_PRED_NET, negate, and / or /
 * implies trees); the watches share the settings' 64 program steps, 16-deep stack and
 * DSL_MAX_NET_CONDS_TOTAL network conditions, and whichever of dsl_set_settings / dsl_set_watches
 * comes second and makes a sum overflow is refused (DSL_ERR_ARG; the engine keeps what it had).
 * BFS on one shard only: dsl_run with watches and virtual_shards > 1 or world_size > 1 returns
 * DSL_ERR_ARG before any collective. dsl_run_dfs, dsl_replay and dsl_human_readable_trace ignore
 * the watches and report none. */
#define DSL_MAX_WATCHES 8
/* Replaces the engine's watches (n_watches = 0 clears them). `pool` holds the operands of the
   watches' combinators and the conditions of their network leaves, indexed as dsl_settings.pool is
   (n_pool <= DSL_MAX_POOL). The engine keeps them across dsl_set_settings, like the dropped set. */
int dsl_set_watches(dsl_engine* e, const dsl_predicate* watches, int32_t n_watches,
                    const dsl_predicate* pool, int32_t n_pool);
/* The census of the last dsl_run: per_depth[i] (up to cap entries written, *n_levels = the levels
   there are) = states first discovered at depth initial_depth + i in which watch `watch` held;
   *total also includes a level cut short by the time limit. n_levels = 0 after any other call. */
int dsl_watch_counts(dsl_engine* e, int32_t watch, uint64_t* per_depth, int32_t cap,
                     int32_t* n_levels, uint64_t* total);
/* Witnesses: for every watch that asks for one, dsl_run also returns one state of the first depth
 * at which the watch held in a completed level, with a shortest trace to it (depth -
 * initial_depth events) -- what the reference's goalMatchingState() gives a goal search, without
 * the goal search; the state can be the dsl_set_initial of the next stage. Among the states first
 * discovered at that depth in which the watch held it is the one with the smallest fingerprint,
 * in the (hi, lo) order of dsl_result.terminals, so it depends on no arrival order, buffer size or
 * restart; a state with two parents may be traced through either. A watch that holds on the start
 * state has the start state as its witness, with an empty trace. An exceptional successor is never
 * a witness, and a level cut short by the time limit gives none. Nothing else changes: the same
 * states, per_depth, end condition, terminals, traces, check counts and census with or without
 * witness requests. The level that ends a search with a terminal is a completed level.
 * Bit w of `mask` asks for a witness of watch w. A bit at or above the number of watches is
 * DSL_ERR_ARG (named in dsl_last_error; the engine keeps the mask it had). dsl_set_watches resets
 * the mask to 0. */
int dsl_set_watch_witnesses(dsl_engine* e, uint32_t mask);
/* The witness of watch `watch` from the last dsl_run: *depth = its absolute depth, or -1 when there
   is none (not requested, never held in a completed level, or the last call was not a dsl_run); up
   to cap events written to `trace`, *trace_len = the full length; `state` is filled when len is the
   packed state's size. A null engine or a watch index outside the watches set is DSL_ERR_ARG. */
int dsl_watch_witness(dsl_engine* e, int32_t watch, int32_t* depth, dsl_event* trace, int32_t cap,
                      int32_t* trace_len, uint8_t* state, size_t len);

/* The event census: transitions, where the watches count states. Opt-in, for dsl_run on one shard.
 * For every level whose expansion completed -- a queued level, a do_checks level and the level that
 * ends the search with a terminal included; not a level cut short by max_time_ms, and not the
 * maxDepth frontier, which is not expanded -- row i holds one cell per (handler class, destination
 * node) with four counts of the events applied to the states of depth initial_depth + i:
 *   events      enabled events delivered with a non-null result, exactly as dsl_result.successors
 *               counts them: in a search in which no level was cut short, the events of all rows
 *               and cells sum to `successors`;
 *   noops       successors equal to their parent (no new record, the same node words);
 *   exceptions  events whose handler threw;
 *   fresh       successors that are neither, whose state had not been discovered at any depth
 *               <= initial_depth + i: a read-only lookup in the visited table as it stands before
 *               the level inserts anything. Counted per event -- two events of one level that reach
 *               the same new state are both fresh -- so the number depends on no arrival order,
 *               buffer size, table size or restart. events - noops - exceptions - fresh is the
 *               cell's revisit count.
 * A message's class is its handler class (dsl_event_class_name) and its node the destination; a
 * timer's class is its node's timer class and its node the timer's node. An event whose handler the
 * engine proves idle and skips in a plain search is counted under its real class. Classes are
 * [0, dsl_event_class_count), nodes [0, the protocol's nodes); the other cells of the
 * DSL_EVENT_CLASSES x DSL_EVENT_NODES grid are zero. The search itself is the same with or without
 * the census: states, per_depth, successors, end condition, terminals, traces, check counts, watch
 * census and witnesses (the levels run one by one instead of queued on the device, as with
 * do_checks). A search restarted for table growth counts from zero. dsl_run with the census on and
 * virtual_shards > 1 or world_size > 1 returns DSL_ERR_ARG before any collective. dsl_run_dfs,
 * dsl_replay and dsl_human_readable_trace report no rows. */
#define DSL_EVENT_CLASSES 15
#define DSL_EVENT_NODES 8
typedef struct { uint64_t events, noops, exceptions, fresh; } dsl_event_count;
/* The protocol's handler classes: their number, a class's name (static storage; the message or
   timer names dsl_human_readable_trace prints, joined with '|' where a class holds several; NULL
   outside [0, count) or for an unknown protocol) and whether it is a timer class (1 / 0; negative:
   error). Message classes come first. */
int dsl_event_class_count(const dsl_protocol_desc* proto);
const char* dsl_event_class_name(const dsl_protocol_desc* proto, int32_t cls);
int dsl_event_class_is_timer(const dsl_protocol_desc* proto, int32_t cls);
/* Turns the census on (non-zero) or off. Kept across dsl_set_settings, like the watches. */
int dsl_set_event_census(dsl_engine* e, int32_t on);
/* Row `level` of the last dsl_run: DSL_EVENT_CLASSES * DSL_EVENT_NODES cells, class-major, written
   to `cells` unless it is NULL; *n_levels = the rows there are (0 after any other call, or without
   the census). A null engine, or a level outside [0, n_levels) with non-null cells, is DSL_ERR_ARG
   (named in dsl_last_error). */
int dsl_event_census(dsl_engine* e, int32_t level, dsl_event_count* cells, int32_t* n_levels);

/* Step invariants: predicates over an edge (P, E, X) -- P a state the BFS expands, E one of its
 * enabled events, X the successor -- where an invariant is a predicate over one state. Opt-in, for
 * dsl_run on one shard.
 * Judged edges: every edge whose handler returns normally and whose successor differs from its
 * parent (the event census's events - noops - exceptions). A stuttering step (X == P) is exempt, an
 * exceptional step has no successor and is not judged; an edge is judged whether X is new, already
 * visited, pruned, a goal or a maxDepth state. The unexpanded maxDepth frontier has no outgoing
 * edges; the start state has no incoming one.
 * A step invariant whose value is false, or that threw, is violated. The search ends at the first
 * level with a violated edge, and that level is completed as always. Priority within the level:
 * EXCEPTION > state INVARIANT > step INVARIANT > GOAL. When the level's best terminal is an
 * exception or a state invariant it is reported exactly as without step invariants (and
 * dsl_step_violation still answers). Otherwise end_condition = DSL_INVARIANT_VIOLATED,
 * terminal_depth = depth(P) + 1 (also when X was first discovered shallower), predicate_index =
 * n_invariants + s for the lowest violated step invariant s of the reported edge, the trace is a
 * shortest trace of P followed by E, terminal_state is X, and with max_terminals > 0 the list is
 * that terminal alone (terminals_total = 1).
 * The reported edge is, among the level's violating edges, the one with the smallest (P's
 * fingerprint hi, lo, event index): it depends on no arrival order, chunking, table size or restart.
 * Step invariants that hold change nothing: the same states, per_depth, end condition, terminals,
 * traces, watch counts, witnesses and census (the levels run one by one, as with the census). A
 * restarted search counts from zero. The pass has no deadline check of its own: a violation found
 * in a level that max_time_ms then cuts short is reported, and that level has no edge row.
 * Inside a step invariant: the three step leaves, DSL_PRED_FIELD and the protocol's named leaves
 * (both evaluated on X), negate and the combinators; DSL_PRED_NET is refused (DSL_ERR_ARG).
 * dsl_run with step invariants and virtual_shards > 1 or world_size > 1 returns DSL_ERR_ARG before
 * any collective. dsl_run_dfs, dsl_replay and dsl_human_readable_trace ignore them. */
#define DSL_MAX_STEP_INVARIANTS 8
/* Replaces the engine's step invariants (n = 0 clears them); `pool` as for dsl_set_watches. Kept
   across dsl_set_settings. They share the 64 program steps, the 16-deep stack and the
   DSL_MAX_NET_CONDS_TOTAL conditions with the settings and the watches; whichever call makes a sum
   overflow is refused (DSL_ERR_ARG) and the engine keeps what it had. */
int dsl_set_step_invariants(dsl_engine* e, const dsl_predicate* preds, int32_t n, const dsl_predicate* pool,
                            int32_t n_pool);
/* Edges judged per completed level of the last dsl_run: per_level[i] (up to cap written, *n_levels =
   the rows there are, one per level as the census's rows) for the parents of depth initial_depth + i;
   *total their sum. No rows after any other call or without step invariants. */
int dsl_step_edges(dsl_engine* e, uint64_t* per_level, int32_t cap, int32_t* n_levels, uint64_t* total);
/* The step violation of the last dsl_run: *index = the lowest violated step invariant of the
   reported edge, or -1 when there is none or the last call was not a dsl_run; *depth = depth(P) + 1;
   *edges_violating = the level's violating edges; per_invariant[s] = those violating step invariant
   s (an edge counts for every one it violates); up to cap events of the trace (which ends with E)
   written to `trace`, *trace_len = its full length; parent_state / state = P / X, filled when len is
   the packed state's size. Any out pointer may be NULL. */
int dsl_step_violation(dsl_engine* e, int32_t* index, int32_t* depth, uint64_t* edges_violating,
                       uint64_t per_invariant[DSL_MAX_STEP_INVARIANTS], dsl_event* trace, int32_t cap,
                       int32_t* trace_len, uint8_t* parent_state, uint8_t* state, size_t len);

/* Random depth-first search (Search.dfs / RandomDFS, Search.java:397-402, :507-583): `probes`
 * independent random walks run concurrently on the device (one per lane), each restarted from
 * the initial state when it ends, until a terminal state is found (EXCEPTION / INVARIANT / GOAL,
 * with its replayable trace) or the time (settings.max_time_ms) or probe budget is spent
 * (end condition TIME_EXHAUSTED: RandomDFS never exhausts the space). result->states counts the
 * initial state once per probe plus every non-null successor, as RandomDFS does; per_depth is
 * empty. Single shard only. */
typedef struct {
  int64_t probes;           /* concurrent walks (0 = 65536) */
  uint64_t seed;
  int64_t max_probes;       /* stop after this many probes were started (0 = no limit) */
  int32_t steps_per_launch; /* 0 = 64 */
  int32_t max_trace;        /* events recorded per probe when maxDepth is unbounded (0 = 4096) */
  int32_t no_minimize;      /* 0: the terminal's trace is minimized, as RandomDFS does
                               (checkState(s, true), Search.java:570); 1: the probe's raw trace */
  int32_t reserved;
} dsl_dfs_config;

int dsl_run_dfs(dsl_engine* e, const dsl_dfs_config* cfg, dsl_result** out);

/* Trace replay (TraceReplaySearch.replayTrace, T/junit/TraceReplaySearch.java:76-101): steps
 * `trace` from the initial state under the settings -- every event must be deliverable in the
 * state it is applied to (stepEvent with skipChecks = false, SearchState.java:282-359) -- and runs
 * checkState after each step. The first TERMINAL state ends the replay; with `minimize` its trace
 * is minimized (TraceMinimizer.minimizeTrace / minimizeExceptionCausingTrace,
 * T/search/TraceMinimizer.java:32-108) while the reported predicate stays the one that fired. An
 * event that cannot be delivered, or the end of the trace, gives SPACE_EXHAUSTED with the last
 * state reached. Events are matched by content (dsl_event fields, reserved ignored). Runs on the
 * host over the same packed transition functions as the device kernels. */
int dsl_replay(dsl_engine* e, const dsl_event* trace, int32_t n, int32_t minimize, dsl_result** out);

/* SearchState.humanReadableTrace (T/search/SearchState.java:373-470): the events of `trace` (from
 * the initial state) reordered along their causal graph -- a message's first sender before its
 * delivery, each node's steps in order -- depth-first, replayed without delivery checks, steps
 * that leave the state unchanged dropped. Where the reference iterates a HashSet (unspecified
 * order), ready successors are taken in trace order. out->trace is the new trace, terminal_state
 * its end state (equal to the original end state); end_condition is SPACE_EXHAUSTED. Host side. */
int dsl_human_readable_trace(dsl_engine* e, const dsl_event* trace, int32_t n, dsl_result** out);
/* Cumulative kernel statistics of the last dsl_run (HIP events on the engine's stream). The
 * byte model of the expand kernel: parents read once (S bytes each), one 64-byte
 * visited-table bucket line per successor probe, one bucket line written back + 12 bytes of
 * parent/event per newly discovered state, S bytes per successor appended to the next frontier. */
typedef struct {
  double expand_ms;          /* sum of k_level durations (HIP events on the engine's stream) */
  double exchange_ms;        /* host wall time of the multi-shard exchange phases (0 on one shard) */
  uint64_t expand_launches;
  uint64_t parents;          /* frontier states expanded */
  uint64_t work_items;       /* (state, event) pairs = successors generated */
  uint64_t new_states;       /* newly discovered successors */
  uint64_t appended;         /* VALID successors written to the next frontier */
  uint64_t exchanged;        /* successors routed to another shard */
  uint32_t state_bytes;
  uint32_t world_size;
  uint64_t table_slots;
  uint64_t terminal_finds;   /* levels whose best terminal was resolved by a find-mode re-run */
  uint64_t sharded_levels;   /* levels expanded hash-sharded with an exchange (multi-shard) */
  uint64_t probes;           /* visited-table probes: successors that are not no-ops (an event that
                                changes neither its node nor the network leads back to its parent) */
  uint64_t host_syncs;       /* host round trips of the search: stream synchronizations and collectives */
  uint64_t table_rehashes;   /* visited-table growths (rehashed into a table twice the size) */
  int32_t rccl_version;      /* ncclGetVersion() of the RCCL the engine bound (multi-GPU), 0 otherwise */
  int32_t level_slots;       /* k_level workgroups resident at once (occupancy x CUs): the grid of a level */
  /* multi-shard cost model (replicate_below = -1), as agreed by the ranks for this search: k_level ns
     per work item, the non-kernel time of a sharded level (us; 0 = not measured yet, defaults used),
     and the resulting work threshold above which a level is sharded */
  double cost_c_ns;
  double cost_x_us;
  uint64_t shard_work_min;
  /* sharded levels: all-to-all rounds run, levels completed in ONE host round trip (the slab fast
     path), and levels that needed the completion phase (a slab or a region overflowed) */
  uint64_t exchange_rounds;
  uint64_t fast_levels;
  uint64_t completions;
  uint64_t deduped; /* reserved, always 0 */
} dsl_stats;

int dsl_kernel_stats(dsl_engine* e, dsl_stats* out);

/* Caller-provided transport for a multi-process search (one shard per process), used instead
 * of RCCL: e.g. MPI, a JVM-side transport, or torch.distributed/gloo in tests. All buffers are
 * HOST memory; every callback is collective (all ranks call it in the same order) and returns 0
 * on success. alltoallv: send_bytes[d] bytes at send + send_off[d] go to rank d; recv_bytes[s]
 * bytes from rank s land at recv + recv_off[s]. */
typedef struct {
  void* ctx;
  int32_t rank, size;
  int (*allgather_u64)(void* ctx, const uint64_t* in, int32_t n, uint64_t* out /* size*n */);
  int (*allreduce_u64)(void* ctx, uint64_t* v, int32_t n, int32_t is_min);
  int (*bcast_u64)(void* ctx, uint64_t* v, int32_t n, int32_t root);
  int (*alltoallv)(void* ctx, const uint8_t* send, const uint64_t* send_off, const uint64_t* send_bytes,
                   uint8_t* recv, const uint64_t* recv_off, const uint64_t* recv_bytes);
  int32_t flags;            /* DSL_HOST_COMM_* */
  int32_t reserved;
} dsl_host_comm;

/* dsl_host_comm.flags */
#define DSL_HOST_COMM_DEVICE_COLLECTIVES 1 /* the engine takes its RCCL code path (device-side gathers of
                                              the route counts and the level records, enqueued on its
                                              stream); the transport emulates each device gather as a
                                              copy to the host, allgather_u64 and a copy back (tests) */

int dsl_create_with_host_comm(const dsl_protocol_desc* proto, const dsl_engine_config* cfg,
                              const dsl_host_comm* comm, dsl_engine** out);
void dsl_result_free(dsl_result* r);
void dsl_destroy(dsl_engine* e);
const char* dsl_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* DSLABS_HIP_H_ */
