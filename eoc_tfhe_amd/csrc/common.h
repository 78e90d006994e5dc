// common.h -- small shared helpers of the engine and the host-side client code.
#pragma once
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>

// last error message (also echoed on stderr, the reference's convention:
// ao-tfhe/eoc-tfhe-run.cpp:218-219,277-278)
void eoc_set_error(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
// the message is per thread (eoc_last_error reads the calling thread's): a result produced on a worker thread hands its
// message over to the thread that reports the error code (already echoed on stderr once, so not again)
void eoc_adopt_error(const char *msg);

// levels of a netlist as eoc_circuit_run_device evaluates it (host.cpp): RAW, WAR and WAW hazards on wires, 1-based;
// gates must have been checked (valid opcodes, wire ids below n_wires).  Returns the number of levels.
struct eoc_gate;
int eoc_levelise(const eoc_gate *gates, size_t n_gates, size_t n_wires, int *level_of);

// compact public-key lists.  eoc_compact_expand_device with sample 0 at slot `first_slot` of d_lists (counted
// from slot 0 of list 0): what a shard of the global context that starts inside a list needs (engine.hip)
struct eoc_engine;
int eoc_compact_expand_device_from(eoc_engine *e, const int32_t *d_lists, size_t first_slot, size_t count, int32_t *d_out,
                                   void *hip_stream);
// eoc_compact_expand's GPU half on the process-global engines (multi.hip): samples cut into eoc_shard_range blocks, one per
// engine; the caller (host.cpp) has brought the engines up behind the global key
int eoc_compact_expand_engines(const int32_t *lists, size_t count, int32_t *out);
// eoc_table_read's GPU half on the process-global engines (multi.hip): queries cut into eoc_shard_range blocks, one per engine
int eoc_table_read_engines(const int32_t *table, int log2_lists, int log2_width, const int32_t *selectors, size_t queries,
                           int32_t *out);
// eoc_table_update's GPU half on the process-global engines (multi.hip): queries cut into eoc_shard_range blocks,
// one zeroed delta table per engine, added into `table` on the host
int eoc_table_update_engines(int32_t *table, int log2_lists, int log2_width, const int32_t *selectors, const int32_t *values,
                             size_t queries);
// finite automata: the host-side validation every automaton call runs before anything touches a device
// (engine.hip): trans [states][4] = {next0, w0, next1, w1}, starts [n_starts] (may be NULL with n_starts = 0).  EOC_ERR_ARG, with
// the message under the caller's name `who`, for states outside [1, 4096], a successor outside [0, states), a weight outside
// [0, 2N) or a start state outside [0, states)
int eoc_automaton_check(const char *who, const int32_t *trans, size_t states, const int32_t *starts, size_t n_starts);
// eoc_automaton_run's GPU half on the process-global engines (multi.hip): queries cut into eoc_shard_range blocks,
// one per engine; every engine receives the final vector and converts its own selectors
int eoc_automaton_run_engines(const int32_t *trans, size_t states, const int32_t *final_vec, const int32_t *selectors, size_t steps,
                              const int32_t *starts, size_t n_starts, int log2_width, int32_t *out, size_t queries);
// packing key switch: a whole EOCPKS1 blob with t = 4, basebit = 4 -> its parameters and the rows [n][4][2][N]
// in torus form (a pointer into the blob); false for anything else (legacy.cpp)
struct eoc_params;
bool eoc_packing_key_blob_rows(const void *buf, size_t len, eoc_params *p, const int32_t **rows);
// seeded cloud key: a whole EOCCKS1 blob -> its parameters, the 32-byte mask seed and the two body arrays
// (pointers into the blob: BK bodies [n][2l][N], KSK bodies [N t (base - 1)]); false for anything else (legacy.cpp)
bool eoc_seeded_cloud_key_blob_parts(const void *buf, size_t len, eoc_params *p, const uint8_t **seed, const int32_t **bk_bodies,
                                     const int32_t **ksk_bodies);
// eoc_pack's GPU half on the process-global engines (multi.hip): WHOLE lists cut into eoc_shard_range blocks, one per engine
int eoc_pack_engines(const int32_t *cts, size_t count, int32_t *lists);
// eoc_linear's GPU half on the process-global engines (multi.hip): WHOLE input vectors cut into eoc_shard_range
// blocks, one per engine
int eoc_linear_engines(const int8_t *h_w, size_t rows, size_t cols, const int32_t *h_lists, size_t batch, const int32_t *h_bias,
                       int32_t *h_out);
// the packing key on every process-global engine (multi.hip)
int eoc_set_packing_key_engines(const void *blob, size_t len);
// eoc_lut2_batch's GPU half on the process-global engines (multi.hip): rows cut into eoc_shard_range blocks, one
// per engine
int eoc_lut2_engines(int p, int n_tables, const int32_t *tables, size_t n_funcs, const int32_t *x, const int32_t *y, int32_t *out,
                     size_t count);
