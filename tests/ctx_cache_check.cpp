// Stand-alone check of csrc/ctx_cache.hpp (built and run by tests/test_ctx_cache_host.py with the host compiler and its sanitizers).
// Every event is applied to a record with all flags set and to one with all flags clear, and the COMPLETE flag vector is compared
// with what the assignments at that site did before the record existed (commit 276896e: the loose bools of vbmf_ctx).  The
// expectations below were transcribed from those sites, not from the header.  Then the chains that DESIGN.md section 10 promises.
#include <cstdio>
#include <string>
#include <vector>

#include "../vbmatrixfactorization.jl_amd/csrc/ctx_cache.hpp"

using vbmf::CtxCache;

enum : unsigned {
    GA = 1u << 0, GB = 1u << 1, P = 1u << 2, Q = 1u << 3, TR = 1u << 4, G = 1u << 5, W = 1u << 6, OWED = 1u << 7, STALE = 1u << 8,
    FD = 1u << 9, TRYY = 1u << 10, NMEAN = 1u << 11, HAVE_Y = 1u << 12, HAVE_STATE = 1u << 13, HAVE_NOISE = 1u << 14, ALL = (1u << 15) - 1
};
static const char* NAMES[15] = {"gram_A", "gram_B", "P", "Q", "tr", "G", "W", "B_owed", "B32_stale", "delta_tiles", "trYY_reduced",
                                "noise_mean_reduced", "have_Y", "have_state", "have_noise"};

static unsigned bits(const CtxCache& c) {
    const bool v[15] = {c.gram_A(), c.gram_B(), c.P(), c.Q(), c.tr(), c.G(), c.W(), c.B_owed(), c.B32_stale(), c.delta_tiles(),
                        c.trYY_reduced(), c.noise_mean_reduced(), c.have_Y(), c.have_state(), c.have_noise()};
    unsigned b = 0;
    for (int i = 0; i < 15; ++i) b |= v[i] ? 1u << i : 0u;
    return b;
}

static int failures = 0;
static void expect(const std::string& what, unsigned got, unsigned want) {
    if (got == want) return;
    ++failures;
    std::printf("FAIL %s:", what.c_str());
    for (int i = 0; i < 15; ++i)
        if ((got ^ want) & (1u << i)) std::printf(" %s=%d (expected %d)", NAMES[i], (got >> i) & 1, (want >> i) & 1);
    std::printf("\n");
}

static CtxCache all_clear() {
    CtxCache c;                                          // a new context: only trYY_reduced is set
    c.communicator_attached();
    return c;
}
static CtxCache all_set() {
    CtxCache c;
    c.Y_complete(true);
    c.state_set_sparse();
    c.noise_rows_set();
    c.noise_mean_summed();
    c.B_moved_sparse(false);
    c.A_moved_basic();
    c.tr_made();
    c.G_built();
    c.W_made();
    c.gram_run_ended(true, true);
    c.B32_store_skipped();
    c.delta_tiles_written(true);
    return c;
}

struct Event {
    const char* name;                                    // the site at the parent commit
    void (*apply)(CtxCache&);
    unsigned sets, clears;                               // every other flag stays as it was
};

int main() {
    expect("a new context", bits(CtxCache{}), TRYY);
    expect("all clear", bits(all_clear()), 0u);
    expect("all set", bits(all_set()), ALL);

    const std::vector<Event> events = {
        {"vbmf_set_Y_rows, row0 == 0", [](CtxCache& c) { c.Y_begins(); }, 0, HAVE_Y | P | Q | TR | G | W | OWED},
        {"finish_Y, one rank, no communicator", [](CtxCache& c) { c.Y_complete(true); }, HAVE_Y | TRYY, P | Q | TR | G | W | OWED},
        {"finish_Y, sharded or nranks > 1", [](CtxCache& c) { c.Y_complete(false); }, HAVE_Y, TRYY | P | Q | TR | G | W | OWED},
        {"vbmf_set_state", [](CtxCache& c) { c.state_set_basic(); }, HAVE_STATE, GA | GB | P | TR | W | OWED | STALE},
        {"vbmf_sparse_set_state", [](CtxCache& c) { c.state_set_sparse(); }, HAVE_STATE, GA | GB | P | TR | W | OWED | STALE | Q | HAVE_NOISE},
        {"device_err_status, epilogue time-out", [](CtxCache& c) { c.state_mixed(); }, 0, HAVE_STATE},
        {"vbmf_comm_init / vbmf_comm_set_transport", [](CtxCache& c) { c.communicator_attached(); }, 0, TRYY | GA | GB},
        {"do_update_A", [](CtxCache& c) { c.A_moved_basic(); }, GA | P, TR},
        {"do_sparse_update_A, full_cov exit", [](CtxCache& c) { c.A_moved_sparse(true); }, GA | P, Q | TR},
        {"do_sparse_update_A, diagonal exit, homoscedastic", [](CtxCache& c) { c.A_moved_sparse(true); }, GA | P, Q | TR},
        {"do_sparse_update_A, diagonal exit, diag_var", [](CtxCache& c) { c.A_moved_sparse(false); }, GA, P | Q | TR},
        {"vbmf_run_fixed_basis, fast path", [](CtxCache& c) { c.A_moved_by_vbls_loop(); }, GA, TR},
        {"do_update_B, both exits", [](CtxCache& c) { c.B_moved_basic(); }, GB | TR, P},
        {"do_sparse_update_B, homoscedastic", [](CtxCache& c) { c.B_moved_sparse(false); }, GB | Q | TR, P},
        {"do_sparse_update_B, diag_var", [](CtxCache& c) { c.B_moved_sparse(true); }, GB | Q, P | TR},
        {"gram_sweep", [](CtxCache& c) { c.gram_sweep_done_basic(); }, GA | GB | TR, P},
        {"sparse_gram_sweep", [](CtxCache& c) { c.gram_sweep_done_sparse(); }, GA | GB | TR, P | Q},
        {"run loops, after the streaming sweep's gram_product", [](CtxCache& c) { c.W_made(); }, W, 0},
        {"vbmf_step and the other W drops", [](CtxCache& c) { c.W_dropped(); }, 0, W},
        {"gram_prepare, buffers allocated", [](CtxCache& c) { c.G_buffers_new(); }, 0, G},
        {"gram_prepare, G built", [](CtxCache& c) { c.G_built(); }, G, W},
        {"vbmf_run: RunFrame::finish and the lines after it", [](CtxCache& c) { c.run_ended_basic(); }, GA | GB | TR, P},
        {"sparse_run_impl: the same, homoscedastic", [](CtxCache& c) { c.run_ended_sparse(false); }, GA | GB | TR, P | Q},
        {"sparse_run_impl: the same, diag_var", [](CtxCache& c) { c.run_ended_sparse(true); }, GA | GB, P | Q | TR},
        {"Gram run failed", [](CtxCache& c) { c.gram_run_ended(false, true); }, 0, W},
        {"Gram run failed before any Gram sweep", [](CtxCache& c) { c.gram_run_ended(false, false); }, 0, W},
        {"Gram run OK, at least one Gram sweep executed", [](CtxCache& c) { c.gram_run_ended(true, true); }, OWED, 0},
        {"Gram run OK, only the streaming sweep executed", [](CtxCache& c) { c.gram_run_ended(true, false); }, 0, 0},
        {"ensure_B, before the pass", [](CtxCache& c) { c.B_payment_begins(); }, 0, OWED},
        {"ensure_B, after the pass, basic", [](CtxCache& c) { c.B_payment_ends(false, true); }, 0, 0},
        {"ensure_B, after the pass, sparse", [](CtxCache& c) { c.B_payment_ends(true, true); }, 0, Q},
        {"ensure_B, failure, basic", [](CtxCache& c) { c.B_payment_ends(false, false); }, 0, W},
        {"ensure_B, failure, sparse", [](CtxCache& c) { c.B_payment_ends(true, false); }, 0, W | Q},
        {"ensure_gram_A", [](CtxCache& c) { c.gram_A_made(); }, GA, 0},
        {"ensure_gram_B", [](CtxCache& c) { c.gram_B_made(); }, GB, 0},
        {"prepare_trYBA", [](CtxCache& c) { c.tr_made(); }, TR, 0},
        {"do_hetero_sigma", [](CtxCache& c) { c.Q_made(); }, Q, 0},
        {"vbmf_sparse_set_SigmaA", [](CtxCache& c) { c.SigmaA_set(); }, 0, TR},
        {"the batched vbls! calls, vbmf_debug_time_pass", [](CtxCache& c) { c.P_overwritten(); }, 0, P},
        {"vbmf_sparse_set_noise_rows", [](CtxCache& c) { c.noise_rows_set(); }, HAVE_NOISE, NMEAN},
        {"ensure_ready, ||Y||^2", [](CtxCache& c) { c.trYY_summed(); }, TRYY, 0},
        {"ensure_ready, mean(sigmaVecHat)", [](CtxCache& c) { c.noise_mean_summed(); }, NMEAN, 0},
        {"launchers with store_fac = 0", [](CtxCache& c) { c.B32_store_skipped(); }, STALE, 0},
        {"rebuild_B32_if_stale", [](CtxCache& c) { c.B32_rebuilt(); }, 0, STALE},
        {"launch_post / launch_post_frag, delta tiles written", [](CtxCache& c) { c.delta_tiles_written(true); }, FD, 0},
        {"launch_post / launch_post_frag, none written", [](CtxCache& c) { c.delta_tiles_written(false); }, 0, FD},
    };
    for (const Event& e : events) {
        for (const unsigned start : {(unsigned)ALL, 0u}) {
            CtxCache c = start ? all_set() : all_clear();
            e.apply(c);
            expect(std::string(e.name) + (start ? " (from all set)" : " (from all clear)"), bits(c), (start | e.sets) & ~e.clears);
        }
    }

    // ---- the chains of DESIGN.md section 10 ----
    auto gram_run = [](CtxCache& c, bool sparse) {       // a run that finds G missing, streams its first sweep and continues in the Gram form
        c.G_buffers_new();
        c.G_built();
        sparse ? c.A_moved_sparse(true) : c.A_moved_basic();
        sparse ? c.B_moved_sparse(false) : c.B_moved_basic();
        c.W_made();
        sparse ? c.gram_sweep_done_sparse() : c.gram_sweep_done_basic();
        sparse ? c.run_ended_sparse(false) : c.run_ended_basic();
        c.gram_run_ended(true, true);
    };
    for (const bool sparse : {false, true}) {
        CtxCache c;
        c.Y_complete(true);
        sparse ? c.state_set_sparse() : c.state_set_basic();
        gram_run(c, sparse);
        const unsigned after_run = HAVE_Y | HAVE_STATE | TRYY | GA | GB | TR | G | W | OWED;
        expect("Gram run -> B owed", bits(c), after_run);
        CtxCache s = c;
        sparse ? s.state_set_sparse() : s.state_set_basic();
        expect("Gram run -> state set -> not owed, W dropped", bits(s), HAVE_Y | HAVE_STATE | TRYY | G);
        CtxCache y = c;
        y.Y_begins();
        expect("Gram run -> Y begins -> G, W dropped, not owed", bits(y), HAVE_STATE | TRYY | GA | GB);
        CtxCache b = c;                                  // the first reader pays; W stays for a run that continues
        b.B_payment_begins();
        sparse ? b.B_moved_sparse(false) : b.B_moved_basic();
        b.B_payment_ends(sparse, true);
        expect("Gram run -> B paid -> W kept", bits(b), after_run & ~OWED);
    }
    {
        CtxCache c;
        c.Y_complete(true);
        c.state_set_sparse();
        c.A_moved_sparse(true);
        c.B_moved_sparse(false);
        expect("A moved -> B moved: tr made", bits(c), HAVE_Y | HAVE_STATE | TRYY | GA | GB | Q | TR);
        c.SigmaA_set();
        expect("A moved -> B moved -> SigmaA set -> tr dropped", bits(c), HAVE_Y | HAVE_STATE | TRYY | GA | GB | Q);
    }
    {
        CtxCache c;
        c.Y_complete(true);
        c.state_set_basic();
        c.A_moved_basic();
        c.B_moved_basic();
        c.communicator_attached();
        expect("communicator attached -> gA, gB dropped, trYY owed", bits(c), HAVE_Y | HAVE_STATE | TR);
        c.trYY_summed();
        c.gram_A_made();
        c.gram_B_made();
        expect("... and paid by the next step", bits(c), HAVE_Y | HAVE_STATE | TR | TRYY | GA | GB);
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ctx_cache: %zu events from both ends and the chains hold\n", events.size());
    return 0;
}
