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
// finite automata: the host-side validation every automaton call runs before anything touches a device
// (engine.hip): trans [states][4] = {next0, w0, next1, w1}, starts [n_starts] (may be NULL with n_starts = 0).  EOC_ERR_ARG, with
// the message under the caller's name `who`, for states outside [1, 4096], a successor outside [0, states), a weight outside
// [0, 2N) or a start state outside [0, states)
int eoc_automaton_check(const char *who, const int32_t *trans, size_t states, const int32_t *starts, size_t n_starts);
// packing key switch: a whole EOCPKS1 blob with t = 4, basebit = 4 -> its parameters and the rows [n][4][2][N]
// in torus form (a pointer into the blob); false for anything else (legacy.cpp)
struct eoc_params;
bool eoc_packing_key_blob_rows(const void *buf, size_t len, eoc_params *p, const int32_t **rows);
// seeded cloud key: a whole EOCCKS1 blob -> its parameters, the 32-byte mask seed and the two body arrays
// (pointers into the blob: BK bodies [n][2l][N], KSK bodies [N t (base - 1)]); false for anything else (legacy.cpp)
bool eoc_seeded_cloud_key_blob_parts(const void *buf, size_t len, eoc_params *p, const uint8_t **seed, const int32_t **bk_bodies,
                                     const int32_t **ksk_bodies);
