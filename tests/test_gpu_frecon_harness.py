"""The round harness's COFIG and FRECON rounds on the product path (HIP codecs in the fused shift
steps, HIP folds) against the reference's runs (tests/golden/harness_frecon.*), compared as
tests/test_gpu_harness.py compares the DIANA runs:
  * device "cpu"  — the reference's --gpu -1 setting: the model side on the host, every codec call
    and both server folds in libflcodec.so;
  * device "cuda" — the whole round on the MI355X.
Per round the history scalars within 1e-6 relative, the clients' f values and wire counts, the
sampling / pattern draw order exact, the server's h_prev after every state update, the iterates, and
every round's model fold bit-exact against the oracle's sequential serverGradient."""
import numpy as np
import pytest
import torch

from oracle import codecs as oc
from tests.frecon_cases import DATA, META, RUN_NAMES, check_h_prev, check_history, simulation

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ag():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from flpytorch_amd import aggregation
    return aggregation


@pytest.mark.parametrize("device", ["cpu", "cuda"])
@pytest.mark.parametrize("name", RUN_NAMES)
def test_harness_reproduces_reference_run(ag, name, device):
    folds = []
    sim = simulation(name, device, record_iterates=True)
    default_fold = sim.server_gradient                    # serverGradientCOFIG / the FRECON wrapper

    def recording_fold(buf, clients, model, x, H):
        rows = [buf.get(i)["model"].detach().cpu().numpy().copy() for i in range(clients)]
        gs = default_fold(buf, clients, model, x, H)
        folds.append((x.detach().cpu().numpy().copy(), rows, H["u_avg_update"].detach().cpu().numpy().copy()))
        return gs
    sim.server_gradient = recording_fold
    hs = []
    for r in range(sim.rounds):
        sim.run_round(r)
        hs.append(sim.H["h_prev"].detach().cpu().numpy().copy())
    check_history(name, sim.H, rel=1e-6)
    check_h_prev(name, hs)
    for r in range(META[name]["rounds"]):
        np.testing.assert_allclose(sim.iterates[r].numpy(), DATA[f"{name}_iterates"][r], rtol=1e-5, atol=1e-6,
                                   err_msg=f"{name} round {r}")
    # the HIP fold of each round's client models, bit for bit the reference's sequential fp32 loop
    for x, rows, u in folds:
        want = oc.server_gradient(x, rows)
        assert np.array_equal(u.view(np.uint32), want.view(np.uint32))
