"""The round harness in resident mode (``Simulation(resident=True)``): the per-client state rows in one
[num_clients, D] device matrix, each local iteration of a round one sampled call over the rows the
sampling picked (the ``_sampled`` entries).  The reference's partial-participation runs (2 of 4
clients per round) are replayed with the checks and tolerances of tests/harness_cases.py and
tests/frecon_cases.py, the ones tests/test_gpu_harness.py and tests/test_gpu_frecon_harness.py apply to
the default mode, and the iterates are those of the default mode bit for bit."""
import numpy as np
import pytest
import torch

from tests import frecon_cases, harness_cases

pytestmark = pytest.mark.gpu

RUNS = {"ef21_randk10_p2": harness_cases, "diana_randk10_p2_li2": harness_cases, "ef21_topk10_p2_li2": harness_cases,
        "cofig_randk10_p2_li2": frecon_cases}


@pytest.fixture(scope="module")
def ag():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from flpytorch_amd import aggregation
    return aggregation


def run(cases, name, device, resident):
    sim = cases.simulation(name, device, record_iterates=True, resident=resident)
    shifts = []
    for r in range(sim.rounds):
        sim.run_round(r)
        algo = cases.META[name]["algorithm"]
        if algo == "diana":
            shifts.append(sim.H["h"].detach().cpu().numpy().copy())
        elif algo == "cofig":
            shifts.append(sim.H["h_prev"].detach().cpu().numpy().copy())
    return sim, shifts


@pytest.mark.parametrize("device", ["cpu", "cuda"])
@pytest.mark.parametrize("name", sorted(RUNS))
def test_resident_mode_reproduces_reference_run(ag, name, device):
    cases = RUNS[name]
    m = cases.META[name]
    assert m["clients_per_round"] < m["num_clients"]             # partial participation
    sim, shifts = run(cases, name, device, True)
    assert sim.resident and tuple(sim.state.shape) == (m["num_clients"], m["D"]) and sim.state.is_cuda
    cases.check_history(name, sim.H, rel=1e-6)
    if m["algorithm"] == "diana":
        harness_cases.check_server_shift(name, shifts)
    elif m["algorithm"] == "cofig":
        frecon_cases.check_h_prev(name, shifts)
    for r in range(m["rounds"]):
        np.testing.assert_allclose(sim.iterates[r].numpy(), cases.DATA[f"{name}_iterates"][r], rtol=1e-5, atol=1e-6,
                                   err_msg=f"{name} round {r}")
    for rec in sim.H["history"].values():                        # the state is in the matrix, not in the records
        for st in rec["client_states"].values():
            assert "hi" not in st["client_state"] and "g_prev" not in st["client_state"]
    # the same run in the default mode: the same iterates and history scalars, exactly
    ref, ref_shifts = run(cases, name, device, False)
    assert not ref.resident
    for r in range(m["rounds"]):
        assert np.array_equal(sim.iterates[r].numpy().view(np.int32), ref.iterates[r].numpy().view(np.int32)), (name, r)
        for k in ("grad_sgd_server_l2", "x_before_round", "approximate_f_avg_value"):
            assert sim.H["history"][r][k] == ref.H["history"][r][k], (name, r, k)
    for a, b in zip(shifts, ref_shifts):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    # and the state rows are what the default mode keeps in its records
    field = "g_prev" if m["algorithm"] == "ef21" else "hi"
    seen = set()
    for r in sorted(ref.H["history"], reverse=True):
        for c, st in ref.H["history"][r]["client_states"].items():
            if c not in seen:
                seen.add(c)
                want = st["client_state"][field]
                assert np.array_equal(sim.state[c].cpu().numpy().view(np.int32), want.cpu().numpy().view(np.int32)), (name, c)


def test_resident_mode_is_refused_elsewhere(ag):
    for name, kw in (("ef21_randk10_p2", {"shift_wire": True}), ("diana_randk10_p2_li2", {"shift_wire": "socket"})):
        with pytest.raises(ValueError, match="resident"):
            harness_cases.simulation(name, "cuda", resident=True, **kw)
    others = [n for n in harness_cases.RUN_NAMES if harness_cases.META[n]["algorithm"] in ("dcgd", "fedavg", "marina")]
    seen = set()
    for name in others:
        algo = harness_cases.META[name]["algorithm"]
        if algo in seen:
            continue
        seen.add(algo)
        with pytest.raises(ValueError, match="resident"):
            harness_cases.simulation(name, "cuda", resident=True)
    frecon = [n for n in frecon_cases.RUN_NAMES if frecon_cases.META[n]["algorithm"] == "frecon"]
    with pytest.raises(ValueError, match="resident"):
        frecon_cases.simulation(frecon[0], "cuda", resident=True)
