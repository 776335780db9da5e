/*
 * gorio_scan_batch.h -- the batched section of the scan pipeline's C ABI (libgorio_amd.so).  include/gorio_scan.h includes this header at
 * its end; handles, status codes and conventions are those of that header.  An extension: the reference processes one message per callback.
 *
 * A batch advances `count` pipelines in lock-step rounds: one set of launches over the members that still take part, one stream
 * synchronisation, then the host parts of those members (REVE bookkeeping and solve, the statistical filter's threshold, the Patchwork++
 * decisions, the DBSCAN queue replay and ranking), each the host function of the single call.  The number of launches and of
 * synchronisations depends on which stages are switched on among the members and on the deepest stage a member reaches, not on `count`
 * (DESIGN.md "Scan pipeline", the round table).
 *
 * DEFINITION.  Member i is left exactly as gorio_scan_load(handles[i], ...) / gorio_scan_run(handles[i], ...) would leave that handle from
 * the same prior state, to the last bit: n_gated, n_valid, every field of gorio_scan_result, codes[i] (what the single gorio_scan_run
 * would have returned), the text of gorio_scan_handle_error, every gorio_scan_get_stage / _get_stage_points / _get_output answer, the
 * Patchwork++ state the next frame starts from, and the handle's three counters.  The hand-offs (gorio_apd_set_*_from_scan,
 * gorio_ndt_set_*_from_scan, gorio_kf_add_from_scan) work on each member as after a single run; each member's output is a cloud of its
 * own with its own search index; single and batched calls may alternate on one handle.
 *
 * Members are independent: their parameters may differ in everything, ang_vel[i] may be NULL, n[i] may be 0.  A member that ends early
 * (ZERO_VELOCITY, EMPTY after any stage, REFUSED by a stage) drops out of the later rounds and disturbs nobody; a refused member's run
 * has consumed its load.
 *
 * RETURN VALUE.  0 when the call itself was valid, whatever the members' outcomes (those are in results[i].status and codes[i]).
 * Argument and state errors are reported before any device call and change no handle; gorio_scan_last_error names handles[i]:
 *   GORIO_ERR_INVALID      a null pointer, count < 0, a handle listed twice, handles on different devices, a bad stride or sample argument
 *   GORIO_ERR_STATE        gorio_scan_run_batch: a member without a load
 *   GORIO_ERR_UNSUPPORTED  count > GORIO_SCAN_BATCH_MAX, or more than 2^31 - 1 raw points in all
 * count == 0 returns GORIO_OK and touches nothing.  A HIP runtime failure ends the call with GORIO_ERR_NO_DEVICE.
 *
 * Job tables, staging and the combined block-count scan of a batch live in its lead handle, handles[0]; they grow and never shrink.
 * Each member's stage clouds stay in its own handle.  A batch is driven from one thread.
 */
#ifndef GORIO_SCAN_BATCH_H
#define GORIO_SCAN_BATCH_H

#ifdef __cplusplus
extern "C" {
#endif

#define GORIO_SCAN_BATCH_MAX 1024

/* gorio_scan_load for every member: xyz[i] / power[i] / doppler[i] / n[i] / stride_bytes[i] as gorio_scan_load takes them (the three
 * pointers of a member with n[i] == 0 may be NULL); n_gated[count] and n_valid[count] receive the counts. */
int gorio_scan_load_batch(gorio_scan_t* const* handles, int count, const float* const* xyz, const float* const* power, const float* const* doppler, const int* n,
                          const int* stride_bytes, int* n_gated, int* n_valid);

/* gorio_scan_run for every member: sample_idx[i] / n_iter[i] / ang_vel[i] as gorio_scan_run takes them (sample_idx[i] may be NULL when
 * n_iter[i] is 0; ang_vel, or any ang_vel[i], may be NULL); results[count] and codes[count] receive each member's result and return code. */
int gorio_scan_run_batch(gorio_scan_t* const* handles, int count, const unsigned int* const* sample_idx, const int* n_iter, const double* const* ang_vel,
                         gorio_scan_result* results, int* codes);

/* The text of this handle's last run (single or batched) when it ended REFUSED, "" otherwise.  Valid until the handle's next run. */
const char* gorio_scan_handle_error(const gorio_scan_t* h);

/* Shape of the last batch call (load or run) whose handles[0] was `lead`: rounds that had a member in them, kernel launches and stream
 * synchronisations of the call.  Zeros before the first batch call.  Any output pointer may be NULL. */
int gorio_scan_batch_diag(const gorio_scan_t* lead, int* rounds, int* launches, int* synchronisations);

#ifdef __cplusplus
}
#endif
#endif /* GORIO_SCAN_BATCH_H */
