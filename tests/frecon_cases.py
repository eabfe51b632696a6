"""Shared setup of the COFIG / FRECON round-harness tests: the reference runs captured by
tests/golden/make_golden_frecon.py (harness_frecon.json / harness_frecon.npz) replayed through
flpytorch_amd.harness.Simulation, compared the way tests/harness_cases.py compares the DIANA runs."""
import numpy as np

from tests.golden_io import load

META, DATA = load("harness_frecon")
RUN_NAMES = sorted(META)


def simulation(name, device, **kw):
    from flpytorch_amd import harness
    m = META[name]
    model = harness.DenseModel(DATA["data_A"], DATA["data_B"], m["samples_per_client"])
    assert model.D == m["D"]
    return harness.Simulation(m["algorithm"], m["client_compressor"], model, DATA[f"{name}_x0"], m["num_clients"],
                              m["clients_per_round"], m["rounds"], m["local_lr"], m["global_lr"],
                              local_iters=m["local_iters"], runtime_seed=m["manual_runtime_seed"], device=device,
                              initialize_shifts_policy=m["initialize_shifts_policy"],
                              sampling=m["client_sampling_type"], poisson_p=m["client_sampling_poisson"],
                              algorithm_options=m["algorithm_options"], **kw)


def run_collecting_h_prev(sim):
    """sim.run(), keeping the server's h_prev after every round's state update."""
    hs = []
    for r in range(sim.rounds):
        sim.run_round(r)
        hs.append(sim.H["h_prev"].detach().cpu().numpy().copy())
    return sim.H, hs


def check_h_prev(name, rounds_h, rtol=1e-5, atol=1e-7):
    """The server shift h_prev after each round's serverGlobalStateUpdate (algorithms.py:1181, 1312)
    against the reference run's, with check_server_shift's tolerances."""
    want = DATA[f"{name}_h_prev"]
    assert len(rounds_h) == len(want)
    for r, (got, w) in enumerate(zip(rounds_h, want)):
        np.testing.assert_allclose(got, w, rtol=rtol, atol=atol, err_msg=f"{name} h_prev after round {r}")


def check_history(name, H, rel=1e-6):
    """tests/harness_cases.check_history over this fixture set."""
    want = META[name]["history"]
    assert len(H["history"]) == len(want)
    for r, w in enumerate(want):
        got = H["history"][r]
        assert list(got["client_states"]) == w["clients"], (name, r)
        for c, fv, snd in zip(w["clients"], w["approximate_f_value"], w["send_scalars_to_master"]):
            cs = got["client_states"][c]["client_state"]
            np.testing.assert_allclose(cs["approximate_f_value"], fv, rtol=rel, err_msg=f"{name} r{r} c{c} f")
            assert cs["stats"]["send_scalars_to_master"] == snd, (name, r, c)
        for k in ("grad_sgd_server_l2", "x_before_round", "approximate_f_avg_value"):
            assert abs(got[k] - w[k]) <= rel * abs(w[k]), (name, r, k, got[k], w[k])
