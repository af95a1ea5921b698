/* mplx_multi.h -- Q searches in one node table and one open set (include/mplx_table.h, include/mplx_open.h): many
 * start / goal queries on one map share every launch of a round.  The expansion kernels read one map and one control
 * table and do not care whose node they expand, mplx_table_relax_device takes whatever lists it is given and the passes
 * of a select are O(nodes); what this header adds is the way to keep the queries apart.  Exported by libmplx.so next to
 * include/mplx.h, whose ABI version it does not change.  Nothing here changes a table of one query: mplx_table_create
 * is Q = 1, and mplx_table_create_multi with n_queries == 1 is that call (query_slots_log2 as its slots_log2).
 *
 * Identity.  A node belongs to exactly one query q in [0, Q); its identity is the pair (q, lattice hash).  Two queries
 * never share a node, whatever their hashes -- exactly: q is not folded into a 64-bit key.  Node ids stay global, dense
 * and in entry order across all queries; every node array of mplx_table_view is shared and node_capacity is the total.
 * One more column, int32 query[id] (mplx_table_query_of), says whose a node is.
 *
 * mplx_table_relax_device keeps its signature.  On a table with Q > 1 the query of list row k is query[parent_id[k]],
 * and a row whose parent_id[k] is not the id of a node that existed before the call does not count: it touches nothing.
 * Everything else is the rule of mplx_table.h with "hash" read as "(q, hash)": nodes are created in the order of the
 * smallest counting e that carries their (q, hash), g improves strictly, ties go to the smallest e, the frontier is in
 * the order of the winning e, parent_g is a snapshot.  mplx_table_seed_multi does the same with h_query[i] as the query
 * of seed i and the seed order as e.  mplx_table_path, _view_of, _stats and _clear are unchanged: they work on ids.
 *
 * Realisation and capacity.  Every query has its own region of 2^query_slots_log2 slots of the hash table, probed from
 * mix(hash) inside the region, and its own dedicated slot for the hash equal to the empty marker; the key compare stays
 * the hash alone, because a region holds one query.  query_slots_log2 = 0: the smallest power of two >=
 * 2 * ceil(node_capacity / Q) per query, never fewer than 64.  A query whose region is full (every slot holds another
 * key of that query) raises MPLX_TABLE_PROBE_FULL | MPLX_TABLE_NODES_FULL, sticky, with the consequences mplx_table.h
 * states, even while the node arrays have room; the probe loop is bounded by the region's length and no call writes
 * outside an array.
 *
 * The open set of such a table has one goal per query (mplx_open_set_goals; the goals are copied).
 * mplx_open_push_device keeps its signature: a row's heuristic, tolerance test and (sight != 0) ray of env_map.h:38-43
 * use goals[query[id]].  An open set of a table with one query reads the context's goal (mplx_set_goal) exactly as
 * before, unless mplx_open_set_goals gave it one of its own.
 *
 * mplx_open_select_multi_device applies the rule of mplx_open.h per query: with O_q / G_q the open / goal-region nodes
 * of query q, every query gets its own f_min, goal_f, goal_id (a global id), goal_g, status and threshold
 * T_q = f_min_q + delta.  The selected set is the union of the sets of the queries whose status is
 * MPLX_OPEN_SELECTED; it goes to d_out in ascending global id and is cut to d_out->capacity in that order (the rest
 * stay open: no error, no status bit).  results[q].count = the rows of query q in d_out, results[q].n_open = that
 * query's open nodes after the call, *d_out->count = the total.  A query that is MPLX_OPEN_FOUND or MPLX_OPEN_EMPTY
 * selects nothing, is not disturbed by the others, and its result is the same in every later call.  Every output is a
 * pure function of the inputs.  h_results_or_null != NULL reads Q results (Q * 48 bytes) back with one synchronisation.
 *
 * Errors, beyond those of the two headers: MPLX_ERR_ARG for n_queries outside [1, 65536], for Q * 2^query_slots_log2 +
 * Q >= 2^32 - 1 (slot indices are 32 bits), for a query of a seed or of mplx_table_find_multi outside [0, Q)
 * (mplx_table_find_multi_device answers -1 for such a query), for mplx_open_set_goals with n != Q; MPLX_ERR_STATE for
 * mplx_table_seed, mplx_table_find, mplx_table_find_device and mplx_open_select_device on a table with Q > 1 and for a
 * push on such a table before mplx_open_set_goals.  The _multi calls accept a table of one query (all queries 0) and
 * then give the bytes of the plain calls.                                                                            */
#ifndef MPLX_MULTI_H
#define MPLX_MULTI_H

#include "mplx_open.h"

#ifdef __cplusplus
extern "C" {
#endif

int mplx_table_create_multi(mplx_ctx *ctx, int64_t node_capacity, int32_t n_queries, int32_t query_slots_log2, mplx_table **out);
/* The per-node query column (device memory of the table, [node_capacity], rows [0, n_nodes) valid) and Q.  A table of
 * one query has no column: *d_query = NULL, every node's query is 0.  Either pointer may be NULL, not both.         */
int mplx_table_query_of(mplx_table *tab, const int32_t **d_query, int32_t *n_queries);
/* mplx_table_seed with h_query[n], the query of every seed.                                                         */
int mplx_table_seed_multi(mplx_table *tab, const double *h_states, int64_t n, int64_t stride, const double *h_g_or_null,
                          const int32_t *h_query, const mplx_table_frontier *d_frontier, int64_t *h_count_or_null);
/* id of every (query, hash), -1 for a pair the table does not hold.  The host form synchronises.                    */
int mplx_table_find_multi_device(mplx_table *tab, const uint64_t *d_hash, const int32_t *d_query, int64_t n, int32_t *d_id);
int mplx_table_find_multi(mplx_table *tab, const uint64_t *h_hash, const int32_t *h_query, int64_t n, int32_t *h_id);

/* h_goals[n], n == Q of the open set's table; host pointers, staged through the context's arena; synchronises.      */
int mplx_open_set_goals(mplx_open *o, const mplx_goal_spec *h_goals, int32_t n);
/* d_results_or_null / h_results_or_null: Q results each.                                                            */
int mplx_open_select_multi_device(mplx_open *o, double delta, const mplx_table_frontier *d_out,
                                  mplx_open_result *d_results_or_null, mplx_open_result *h_results_or_null);

#ifdef __cplusplus
}
#endif
#endif
