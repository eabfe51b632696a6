#!/usr/bin/env python3
"""Generate the COFIG / FRECON round-harness fixtures (tests/golden/harness_frecon.npz +
harness_frecon.json) from the REAL reference.

Test infrastructure only, built like make_golden_harness.py (same stubs, same ``COMMON`` arguments,
same recorded fields; see its docstring): it runs where the reference is mounted, the GPU box
receives only the fixtures.  On top of make_golden_harness.py's fields it records the server shift
``H['h_prev']`` after every round's serverGlobalStateUpdate (algorithms.py:1181, 1312) and the
run's ``--algorithm-options`` (FRECON's ``lambda_``).

Runs: COFIG (randk, partial participation with 2 local steps, so clients come back to their stored
shifts) and FRECON (qsgd with partial participation; randk with full-gradient initial shifts, which
also start ``g_server_prev`` at the gradient of the whole train set).
"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (stubs, COMMON, REF)

RUNS = {
    "cofig_randk10_p2_li2": ["--algorithm", "cofig", "--client-compressor", "randk:10%",
                             "--num-clients-per-round", "2", "-li", "2", "--rounds", "5"],
    "frecon_qsgd10_p2": ["--algorithm", "frecon", "--client-compressor", "qsgd:10",
                         "--num-clients-per-round", "2", "--rounds", "5",
                         "--algorithm-options", "internal_sgd:full-gradient,lambda_:0.5"],
    "frecon_randk10_fullgrad": ["--algorithm", "frecon", "--client-compressor", "randk:10%",
                                "--initialize-shifts-policy", "full_gradient_at_start", "--rounds", "3",
                                "--algorithm-options", "internal_sgd:full-gradient,lambda_:0.25"],
}


def main():
    tmp = tempfile.mkdtemp(prefix="flstubs_")
    mg._write_stubs(tmp)
    sys.path.insert(0, tmp)
    sys.path.insert(0, os.path.join(mg.REF, "utils"))
    sys.path.insert(0, mg.REF)
    sys.dont_write_bytecode = True
    scratch = tempfile.mkdtemp(prefix="flharness_")
    work = os.path.join(scratch, "a", "b")
    os.makedirs(work)
    os.chdir(work)
    import run as refrun                                  # reference modules, imported read-only
    from utils import algorithms, execution_context
    from models import mutils
    from data_preprocess import artificial_dataset

    iterates, starts, shifts = [], [], []
    orig_sgsu = algorithms.serverGlobalStateUpdate

    def sgsu_wrap(clients_responses, model, *a, **k):
        iterates.append(mutils.get_params(model).detach().cpu().numpy().copy())
        Hn = orig_sgsu(clients_responses, model, *a, **k)
        shifts.append(Hn["h_prev"].detach().cpu().numpy().copy())        # h_prev after its update
        return Hn
    algorithms.serverGlobalStateUpdate = sgsu_wrap
    execution_context.simulation_start_fn = lambda H: starts.append(H["x0"].detach().cpu().numpy().copy())

    captured = []
    orig_init = artificial_dataset.ArificialDataset.__init__

    def init_wrap(self, exec_ctx, args, train=None, *a, **k):
        orig_init(self, exec_ctx, args, train, *a, **k)
        if train is None or train:
            captured.append((self.data.numpy().copy(), self.targets.numpy().copy(), self.n_client_samples))
    artificial_dataset.ArificialDataset.__init__ = init_wrap

    arrays, meta = {}, {}
    for name, extra in RUNS.items():
        captured.clear()
        iterates.clear()
        starts.clear()
        shifts.clear()
        result = {}
        execution_context.simulation_finish_fn = lambda H, _r=result: _r.update(H=H)
        argv = list(mg.COMMON)                 # (a run's own --algorithm-options comes later and wins)
        refrun.runSimulation(argv + extra + ["--run-id", name])
        H = result["H"]
        A, B, S = captured[0]
        if "data_A" in arrays:
            assert np.array_equal(arrays["data_A"], A) and np.array_equal(arrays["data_B"], B)
        arrays["data_A"], arrays["data_B"] = A, B
        arrays[f"{name}_x0"] = starts[0]
        arrays[f"{name}_iterates"] = np.stack(iterates)            # x after each round's global step
        arrays[f"{name}_h_prev"] = np.stack(shifts)
        hist = H["history"]
        rounds = []
        for r in sorted(hist):
            cs = hist[r]["client_states"]
            order = list(cs.keys())
            rounds.append({
                "clients": [int(c) for c in order],
                "approximate_f_value": [[float(v) for v in cs[c]["client_state"]["approximate_f_value"]] for c in order],
                "send_scalars_to_master": [float(cs[c]["client_state"]["stats"]["send_scalars_to_master"]) for c in order],
                "grad_sgd_server_l2": float(hist[r]["grad_sgd_server_l2"]),
                "x_before_round": float(hist[r]["x_before_round"]),
                "approximate_f_avg_value": float(hist[r]["approximate_f_avg_value"]),
            })
        args = H["args"]
        meta[name] = {
            "argv": argv + extra,
            "algorithm": args.algorithm, "client_compressor": args.client_compressor,
            "num_clients": int(H["total_clients"]), "clients_per_round": int(args.num_clients_per_round),
            "rounds": int(args.rounds), "local_iters": int(args.number_of_local_iters),
            "local_lr": float(args.local_lr), "global_lr": float(args.global_lr),
            "manual_runtime_seed": int(args.manual_runtime_seed), "samples_per_client": int(S),
            "D": int(H["D"]), "history": rounds,
            "initialize_shifts_policy": args.initialize_shifts_policy,
            "client_sampling_type": args.client_sampling_type,
            "client_sampling_poisson": float(args.client_sampling_poisson),
            "algorithm_options": args.algorithm_options,
        }
        print(name, [r["grad_sgd_server_l2"] for r in rounds])
    np.savez_compressed(os.path.join(HERE, "harness_frecon.npz"), **arrays)
    with open(os.path.join(HERE, "harness_frecon.json"), "w") as f:
        json.dump(meta, f, indent=1)


if __name__ == "__main__":
    main()
