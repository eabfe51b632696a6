"""CPU tests of the round harness's COFIG and FRECON rounds (flpytorch_amd/harness.py) — the
orchestration, not the kernels: server and client state, the second gradient at x_prev, the two
messages per local iteration on the wire count, lambda_ from the algorithm options, and the
h_prev / x_prev / g_server_prev updates, against the reference's own runs
(tests/golden/harness_frecon.json, from make_golden_frecon.py).

Driven like tests/test_harness.py, with doubles of the codec, step and fold protocols backed by the
oracle.  The product path is tests/test_gpu_frecon_harness.py.
"""
import numpy as np
import pytest
import torch

from tests.frecon_cases import DATA, META, RUN_NAMES, check_h_prev, check_history, run_collecting_h_prev, simulation
from tests.test_harness import OracleCompressorDouble, oracle_diana_step, oracle_server_gradient


def oracle_frecon_step(comp, g, h, g_old, alpha):
    u, h_new = oracle_diana_step(comp, g, h, alpha)                      # algorithms.py:1104-1107
    q = comp.compressVector(g - g_old)                                   # algorithms.py:1116
    return u, h_new, q


def oracle_server_gradient_cofig(buf, clients, model, x, H):
    u = oracle_server_gradient(buf, clients, model, x, H)
    H["u_avg_update"] = u
    H["alpha_update"] = buf.get(0)["client_state"]["alpha"] * (clients / H["total_clients"])
    return u + H["h_prev"]                                               # algorithms.py:1301-1307


def oracle_server_gradient_frecon(buf, clients, model, x, H):
    u = oracle_server_gradient(buf, clients, model, x, H)
    w = buf.get(0)["client_state"]["weight"]
    q_avg = w * buf.get(0)["client_state"]["qi"]                         # algorithms.py:1136-1154
    w_total = w
    for i in range(1, clients):
        cs = buf.get(i)["client_state"]
        q_avg += cs["weight"] * cs["qi"]
        w_total += cs["weight"]
    q_avg = q_avg / w_total
    for i in range(clients):
        del buf.get(i)["client_state"]["qi"]
    lambda_ = float(H["experimental_options"]["lambda_"])
    result = q_avg + (1.0 - lambda_) * H["g_server_prev"] + lambda_ * (u + H["h_prev"])
    H["u_avg_update"] = u
    H["alpha_update"] = buf.get(0)["client_state"]["alpha"] * (clients / H["total_clients"])
    return result


def oracle_simulation(name, **kw):
    fold = {"cofig": oracle_server_gradient_cofig, "frecon": oracle_server_gradient_frecon}[META[name]["algorithm"]]
    return simulation(name, "cpu", init_compressor=OracleCompressorDouble, server_gradient=fold,
                      cofig_step=oracle_diana_step, frecon_step=oracle_frecon_step, **kw)


@pytest.mark.parametrize("name", RUN_NAMES)
def test_harness_replays_reference_runs(name):
    sim = oracle_simulation(name, record_iterates=True)
    H, hs = run_collecting_h_prev(sim)
    check_history(name, H)
    check_h_prev(name, hs)
    for r in range(META[name]["rounds"]):
        np.testing.assert_allclose(sim.iterates[r].numpy(), DATA[f"{name}_iterates"][r], rtol=1e-6, atol=1e-7,
                                   err_msg=f"{name} round {r}")


def test_fixture_covers_both_algorithms_and_returning_clients():
    assert {META[n]["algorithm"] for n in RUN_NAMES} == {"cofig", "frecon"}
    for name in ("cofig_randk10_p2_li2", "frecon_qsgd10_p2"):
        seen, back = set(), False
        for h in META[name]["history"]:
            back |= bool(seen & set(h["clients"]))
            seen |= set(h["clients"])
        assert back, name                                                # a client reads its stored h_i


def test_frecon_counts_two_messages_and_keeps_server_state():
    name = "frecon_qsgd10_p2"
    sim = oracle_simulation(name)
    x0 = sim.x.clone()
    sim.run_round(0)
    comp = OracleCompressorDouble(META[name]["client_compressor"], sim.D)
    comp.generateCompressPattern(np.random.RandomState(0), "cpu", 0, {})
    comp.compressVector(torch.ones(sim.D))
    for st in sim.H["history"][0]["client_states"].values():
        cs = st["client_state"]
        assert cs["stats"]["send_scalars_to_master"] == 2 * META[name]["local_iters"] * comp.last_need_to_send_advance
        assert "qi" not in cs and cs["alpha"] == 1.0 / (1.0 + comp.getW())
    assert torch.equal(sim.H["x_prev"], x0)                               # the round's starting iterate
    assert sim.H["alpha_update"] == cs["alpha"] * (META[name]["clients_per_round"] / META[name]["num_clients"])


def test_frecon_needs_lambda_and_new_algorithms_refuse_the_wire_modes():
    from flpytorch_amd import harness
    m = harness.DenseModel(DATA["data_A"], DATA["data_B"], 16)
    x0 = np.zeros(m.D, np.float32)
    with pytest.raises(ValueError, match="lambda_"):
        harness.Simulation("frecon", "randk:10%", m, x0, 4, 4, 1, 0.1, 1.0, device="cpu")
    for algo in ("cofig", "frecon"):
        for kw in ({"wire": True}, {"shift_wire": True}):
            with pytest.raises(ValueError):
                harness.Simulation(algo, "randk:10%", m, x0, 4, 4, 1, 0.1, 1.0, device="cpu",
                                   algorithm_options="lambda_:0.5", **kw)
    assert harness.parse_algorithm_options("internal_sgd:full-gradient,lambda_:0.5,flag") == \
        {"internal_sgd": "full-gradient", "lambda_": "0.5", "flag": True}
