// ctx_cache.hpp -- which of the data a context derives from (Y, A, B) are current, and the events that change that.
// Plain C++17, no HIP: the host compiler alone builds it (tests/ctx_cache_check.cpp holds every event to its complete flag vector).
//
// vbmf_ctx has one member of this class.  Nothing outside it can write a flag: a call site names what happened, one line, and the
// event says here -- once -- what that makes current and what it drops.  DESIGN.md section 10, "Run boundaries", has the reasoning
// and the same table in prose.  Siblings that differ stay different (the _basic / _sparse pairs, the arguments): an event was merged
// only where every call site did exactly the same.
//
//   flag                 what is current when it is set
//   gram_A, gram_B       the state's A'A / B'B are of the current AHat / BHat
//   P                    c->P / c->Pred hold Y'B of the current B            Q   c->Q holds Y A of the current A (row-noise update)
//   tr                   st[GX] = tr(B'YA) of the current (AHat, BHat)
//   G                    G = Y'Y is of the current Y
//   W                    B = Y W32g[wcur] and gPQ holds [G W | G D] of that W: the next sweep of a run may take the Gram form
//   B_owed               a Gram-form run has ended and B of its last sweep is not materialised yet (ensure_B pays)
//   B32_stale            a launch inside a run skipped the fp32 store of B: the operand tiles are current, B32 is not
//   delta_tiles          c->FD holds old - new of the B update just enqueued
//   trYY_reduced, noise_mean_reduced    ||Y||^2 / mean(sigmaVecHat) in the state are summed over the ranks
//   have_Y, have_state, have_noise      the caller has supplied them (have_Y: every row block of the current Y has arrived)
#pragma once

namespace vbmf {

class CtxCache {
    bool gram_A_ = false, gram_B_ = false, P_ = false, Q_ = false, tr_ = false;
    bool G_ = false, W_ = false, B_owed_ = false, B32_stale_ = false, delta_tiles_ = false;
    bool trYY_reduced_ = true, noise_mean_reduced_ = false;
    bool have_Y_ = false, have_state_ = false, have_noise_ = false;

public:
    bool gram_A() const { return gram_A_; }
    bool gram_B() const { return gram_B_; }
    bool P() const { return P_; }
    bool Q() const { return Q_; }
    bool tr() const { return tr_; }
    bool G() const { return G_; }
    bool W() const { return W_; }
    bool B_owed() const { return B_owed_; }
    bool B32_stale() const { return B32_stale_; }
    bool delta_tiles() const { return delta_tiles_; }
    bool trYY_reduced() const { return trYY_reduced_; }
    bool noise_mean_reduced() const { return noise_mean_reduced_; }
    bool have_Y() const { return have_Y_; }
    bool have_state() const { return have_state_; }
    bool have_noise() const { return have_noise_; }

    // ---- Y --------------------------------------------------------------------------------------------------------------------
    // the first row block of a new Y: none until its last block has arrived; everything made from the old Y goes, the owed B too
    void Y_begins() {
        have_Y_ = false;
        P_ = Q_ = tr_ = false;
        G_ = W_ = false;
        B_owed_ = false;
    }
    // the last block is in.  alone: one rank and no communicator, so this rank's ||Y||^2 is the whole sum
    void Y_complete(bool alone) {
        trYY_reduced_ = alone;
        have_Y_ = true;
        P_ = Q_ = tr_ = false;
        G_ = W_ = false;                                // G = Y'Y is rebuilt by the next run that takes the Gram form
        B_owed_ = false;                                // ... and B = Y W of the old Y is owed no longer
    }

    // ---- the state ------------------------------------------------------------------------------------------------------------
    // vbmf_set_state: B is no longer Y W, so the next run starts by the streaming path, from the B just set
    void state_set_basic() {
        gram_A_ = gram_B_ = P_ = tr_ = false;
        W_ = false;
        B_owed_ = false;
        B32_stale_ = false;
        have_state_ = true;
    }
    // vbmf_sparse_set_state: the same, and Y A and the rows' noise state go too
    void state_set_sparse() {
        state_set_basic();
        Q_ = false;
        have_noise_ = false;
    }
    // the register epilogue's hand-off timed out mid-sweep: the device state is a mixture until the caller sets it again
    void state_mixed() { have_state_ = false; }
    // vbmf_sparse_set_SigmaA: tr(B'YA) in the state is no longer trusted
    void SigmaA_set() { tr_ = false; }
    // vbmf_sparse_set_noise_rows: this rank's share of the mean is in the state
    void noise_rows_set() {
        have_noise_ = true;
        noise_mean_reduced_ = false;
    }
    // vbmf_comm_init, vbmf_comm_set_transport: sums over this rank's rows become shares.  (P, tr and W stay as they are.)
    void communicator_attached() {
        trYY_reduced_ = false;
        gram_A_ = gram_B_ = false;
    }
    void trYY_summed() { trYY_reduced_ = true; }        // ensure_ready
    void noise_mean_summed() { noise_mean_reduced_ = true; }

    // ---- the updates ----------------------------------------------------------------------------------------------------------
    // updateA! formed Y'B and left A'A
    void A_moved_basic() {
        gram_A_ = true;
        P_ = true;
        tr_ = false;
    }
    // P_current: c->Pred is Y'B of the B in the state (not with heteroscedastic rows in the diagonal branch: there it is Y' diag(sigma) B)
    void A_moved_sparse(bool P_current) {
        gram_A_ = true;
        P_ = P_current;
        Q_ = false;
        tr_ = false;
    }
    // the one-workgroup vbls! loop of vbmf_run_fixed_basis moved A from the P of its first iteration
    void A_moved_by_vbls_loop() {
        gram_A_ = true;
        tr_ = false;
    }
    // updateB! left B'B and tr(B'YA) (pair reduce / delta Gram)
    void B_moved_basic() {
        gram_B_ = true;
        P_ = false;
        tr_ = true;
    }
    // ... and Y A of the current A in c->Q; with heteroscedastic rows the trace shares are not formed
    void B_moved_sparse(bool diagvar) {
        gram_B_ = true;
        P_ = false;
        Q_ = true;
        tr_ = !diagvar;
    }
    // a Gram-form sweep moved A and W: the state's sums come from [G W | G D]; c->P is not written
    void gram_sweep_done_basic() {
        gram_A_ = gram_B_ = true;
        P_ = false;
        tr_ = true;
    }
    void gram_sweep_done_sparse() {
        gram_sweep_done_basic();
        Q_ = false;
    }
    void gram_A_made() { gram_A_ = true; }              // ensure_gram_A
    void gram_B_made() { gram_B_ = true; }              // ensure_gram_B
    void tr_made() { tr_ = true; }                      // prepare_trYBA
    void Q_made() { Q_ = true; }                        // do_hetero_sigma
    // a pass wrote c->P with something that is not Y'B of the state's B for the A update (the batched vbls! calls, vbmf_debug_time_pass)
    void P_overwritten() { P_ = false; }

    // ---- the Gram form --------------------------------------------------------------------------------------------------------
    void G_buffers_new() { G_ = false; }                // gram_prepare allocated them
    void G_built() {                                    // ... and built G of the current Y: no W belongs to it yet
        G_ = true;
        W_ = false;
    }
    void W_made() { W_ = true; }                        // a run's streaming sweep was followed by W and [G W | G D]
    // B moved (or may move) without W: steps, vbls!, a run outside the Gram form, a change of form
    void W_dropped() { W_ = false; }

    // ---- run boundaries -------------------------------------------------------------------------------------------------------
    // RunFrame::finish, every path: the last executed sweep left both Grams and tr(B'YA); c->P is of an older B
    void run_ended_basic() {
        gram_A_ = gram_B_ = true;
        P_ = false;
        tr_ = true;
    }
    void run_ended_sparse(bool diagvar) {
        gram_A_ = gram_B_ = true;
        P_ = false;
        Q_ = false;
        tr_ = !diagvar;
    }
    // ... of a run in the Gram form.  swept: the device executed at least one Gram-form sweep, so B of the last one is owed, not made:
    // the first reader pays the pass (ensure_B), a Gram-form run that continues from here never does
    void gram_run_ended(bool ok, bool swept) {
        if (!ok) W_ = false;
        if (ok && swept) B_owed_ = true;
    }
    // ensure_B: the debt is cleared before the pass (the pass's own entry points come back through ensure_B) ...
    void B_payment_begins() { B_owed_ = false; }
    // ... and after it: the sparse B update left Y A of the run's last A in c->Q, which is not what the row-noise update may reuse
    void B_payment_ends(bool sparse, bool ok) {
        if (!ok) W_ = false;
        if (sparse) Q_ = false;
    }

    // ---- the fp32 B and the delta tiles ---------------------------------------------------------------------------------------
    void B32_store_skipped() { B32_stale_ = true; }     // launch_stream's epilogue and the post kernels, inside a run
    void B32_rebuilt() { B32_stale_ = false; }          // rebuild_B32_if_stale
    void delta_tiles_written(bool yes) { delta_tiles_ = yes; }   // the post kernel of a B update
};

}  // namespace vbmf
