/*
 * nabo_potential.h -- C ABI of the differentiation potential of the reference graph in libnabo_knn.so (MI355X,
 * gfx950): one sparse symmetric solve by conjugate gradients with the Jacobi preconditioner.
 *
 * Replaces Graph.calc_diff_potential (nabo/_graph.py:918-954: the population-balance potential of Weinreb et al. 2017;
 * the dense n x n matrix L = I - D^-1 A of refG, numpy.linalg.pinv(L), times r).  The definition below is the
 * specification.  Same conventions as nabo_community.h: 0 or a negative NABO_E_* status, the message
 * in nabo_last_error(), no CPU fallback (NABO_E_NODEVICE without a device).  Every pointer is a host pointer.
 *
 * THE DEFINITION.  Nodes are 0 .. n-1.
 *
 * Graph.  The input is a CSR (ptr, nbr) in either arc direction, made simple: a pair listed more than once counts once,
 * self-loops are kept.  There are no weights (the reference's weight=False).  A_ij = 1 for a listed pair i != j (both
 * ways), A_ii = 1 for a self-loop.  Per node: d_i = sum_j A_ij (a self-loop counts once), c_i = d_i - A_ii.
 * NABO_E_INVALID for a node with d_i = 0 (the reference divides by zero there).
 *
 * Wanted: V = pinv(I - D^-1 A) r.  With K = diag(c) - A_off, the Laplacian of the loop-free graph (symmetric, positive
 * semi-definite), I - D^-1 A = D^-1 K.  Its null space is spanned by the indicators of the connected components of the
 * loop-free graph, the complement of its range by d restricted to each component.  So:
 *
 *   1. label[i] = the smallest node id of the connected component C of i in the loop-free graph.
 *   2. Per component: S1 = sum_C d_i r_i, S2 = sum_C d_i^2 (an exact integer), r'_i = r_i - d_i * (S1 / S2).
 *   3. b_i = d_i * r'_i.  (sum_C b = 0 up to rounding: the system K x = b is consistent.)
 *   4. K x = b by preconditioned conjugate gradients, M = diag(c), 1 / c_i := 0 where c_i = 0; float64 throughout, every
 *      operation rounded once, nothing fused.  Start: x = 0, res = b, p = z = M^-1 res, rho = res^T z, it = 0.  One
 *      iteration:
 *          q_i = c_i p_i - sum_j p_j   (j over the neighbours of i, j != i)
 *          alpha = rho / (p^T q);  x += alpha p;  res -= alpha q;  z = M^-1 res;  rho' = res^T z;
 *          p = z + (rho' / rho) p;  rho = rho';  it += 1.
 *      If p^T q <= 0 or is not finite, the iteration changes nothing and the run stops with status BREAKDOWN.  After
 *      iteration `it` the run stops with status CONVERGED if sqrt(res^T res) <= tol * ||b||_2, else with status MAX_ITER
 *      if it == max_iter.  If ||b||_2 = 0 the run is CONVERGED with x = 0 after 0 iterations.  Once a run has stopped,
 *      further iterations change nothing: the result is the iterate of the first iteration that meets the test.
 *   5. V_i = x_i - (sum_C x) / |C|: the minimum-norm solution, which is what pinv returns.
 *   The true residual ||b - K x||_2 / ||b||_2 is taken with one more product after the loop (0 if ||b||_2 = 0).
 *
 * Every sum is taken in a fixed order -- on the host in ascending node id; on the device per lane, per sub-wave group,
 * per workgroup and over the workgroups' partial sums, all without atomics -- so the same call gives the same bits on
 * every run, however often the host looks at the state in between.  The order itself is not part of the definition.
 */
#ifndef NABO_POTENTIAL_H
#define NABO_POTENTIAL_H

#include <stdint.h>

#include "nabo_knn.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nabo_potential nabo_potential;

#define NABO_POTENTIAL_RUNNING 0
#define NABO_POTENTIAL_CONVERGED 1
#define NABO_POTENTIAL_MAX_ITER 2
#define NABO_POTENTIAL_BREAKDOWN 3

/* The graph (ptr[0] = 0, monotone, every nbr in [0, n); 1 <= n < 2^31), made simple and kept on `device`.  The
 * parameters start as tol = 1e-10, max_iter = 10000. */
int nabo_potential_create(nabo_potential **out, int32_t device, int64_t n, const int64_t *ptr, const int64_t *nbr);
void nabo_potential_destroy(nabo_potential *H);

/* tol finite and >= 0, max_iter >= 1; else NABO_E_INVALID. */
int nabo_potential_set_params(nabo_potential *H, double tol, int64_t max_iter);

/* n nodes, n_arcs off-diagonal arcs (both directions counted), n_long rows of more than long_threshold arcs. */
int nabo_potential_graph_size(nabo_potential *H, int64_t *n, int64_t *n_arcs, int64_t *n_long);

/* Steps 1 - 3 and the start of step 4 for r [n], finite; NULL means all ones. */
int nabo_potential_prepare(nabo_potential *H, const double *r);
/* label [n], d [n], c [n], b [n] of the last prepare (d and c need none); any pointer may be NULL. */
int nabo_potential_get_prepared(nabo_potential *H, int32_t *label, int64_t *d, int64_t *c, double *b);

/* Up to `count` more iterations under the stopping rule; *done != 0 once the run has stopped. */
int nabo_potential_iterate(nabo_potential *H, int64_t count, int32_t *done);
/* x, res, p [n], rho and the number of iterations done; any pointer may be NULL.  set_state (rho finite, it >= 0) puts
 * the run back to RUNNING from the given state. */
int nabo_potential_get_state(nabo_potential *H, double *x, double *res, double *p, double *rho, int64_t *it);
int nabo_potential_set_state(nabo_potential *H, const double *x, const double *res, const double *p, double rho, int64_t it);

/* Step 5 and the true residual from the current x; V [n]. */
int nabo_potential_finish(nabo_potential *H, double *V);
/* prepare, iterate until the run stops, finish. */
int nabo_potential_solve(nabo_potential *H, const double *r, double *V);

/* iterations done, the status, sqrt(res^T res) / ||b|| of the recurrence, the true relative residual of the last finish
 * (-1 before one), the number of components.  Any pointer may be NULL. */
int nabo_potential_info(nabo_potential *H, int64_t *iterations, int32_t *status, double *rel_residual, double *true_residual,
                        int64_t *n_components);

/* The benchmark's timer (tools/bench_potential.py), device ms between HIP events since the last prepare: ms[0] prepare,
 * ms[1] the iterations, ms[2] finish, ms[3] their sum. */
int nabo_potential_last_ms(nabo_potential *H, double ms[4]);

/* How the product is built: `group` lanes share a row of at most `long_threshold` arcs, a longer row takes a workgroup;
 * a workgroup covers `block_rows` consecutive rows and adds their terms of every dot product into one partial sum.
 * Needs no device. */
int nabo_potential_geometry(int32_t *group, int32_t *long_threshold, int32_t *block_rows);

#ifdef __cplusplus
}
#endif

#endif /* NABO_POTENTIAL_H */
