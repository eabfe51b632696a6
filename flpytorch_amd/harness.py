"""The simulated communication round of FL_PyTorch, driven through the MI355X uplink.

The reference's round restated around the product: the host orchestration stays
Python like the reference's, every codec call and the server fold run in libflcodec.so.

  run.py:343-369          np_random.seed(manual_runtime_seed); all rounds' clients pre-sampled
                          (fl_funcs.py:12-43: uniform = choice(n, m, replace=False) per round;
                          poisson = one uniform() per client per round)
  model_funcs.py:459-614  run_one_communication_round: per sampled client, in order,
                          algorithms.clientState (DCGD 1729-1732: initCompressor +
                          generateCompressPattern on the shared stream; then every algorithm's
                          seed draw randint(2**31), algorithms.py:2055) and local_training;
                          then the aggregation block: serverGradient, global optimiser step,
                          serverGlobalStateUpdate
  model_funcs.py:617-723  train_model: per local iteration f, g = local gradient at x_i
                          (algorithms.py:24-113 evaluateGradient, internal_sgd:full-gradient),
                          c = C(g) (DCGD 1735-1745) or g (FedAvg 1797-1807), x_i -= lr * c (SGD,
                          momentum 0: torch.optim.SGD's param.add_(grad, alpha=-lr))
  algorithms.py:2153-2223 serverGlobalStateUpdate: history[round] = {grad_sgd_server_l2 = ||gs||,
                          x_before_round = ||x||, approximate_f_avg_value = mean of the clients'
                          f values, client_states}; l2 = sqrt(sum(v**2).item()) (mutils.py:395)

Where the work runs: the codecs (``Compressor.compressVector``, compat patterns from the shared
numpy stream) and the fold (``serverGradient`` -> flc_reduce_rows) on the GPU, always; the
model-side local gradient (out of the hot path) on the device of the iterate:
``device="cpu"`` mirrors the reference's ``--gpu -1`` runs (config C1: client rows cross to the
GPU for the codec and the fold and back), ``device="cuda"`` keeps the whole round on the MI355X.

Algorithms driven here: DCGD (client step ``C(g)``), FedAvg (``g``), and the shifted ones whose
client step is the fused shift codec (``Compressor.compressShift``, one flc_encode_shift pass):

  DIANA   algorithms.py:1317-1428  h0 = h = 0 or the full gradient at x0 (get_initial_shift,
                                   474-479; run.py:408-418), alpha = 1 / (1 + w); client i keeps
                                   h_i across rounds (findRecentRecordAndRemoveFromHistory,
                                   371-399); step m_i = C(g - h_i), h_i += alpha m_i (dianaStep);
                                   server: gs = fold, H['m'] = gs, returns h + gs, then
                                   h += alpha m
  EF21    algorithms.py:1432-1554  round 0 samples every client (request_use_full_list_of_clients,
                                   model_funcs.py:470-475); a client's first step sends g and keeps
                                   it as g_i; later g_i += C(g - g_i) * mult (ef21Step, mult =
                                   1 / (1 + w) unless C is a contraction); server: fold + master
                                   (identity) compressor

  COFIG   algorithms.py:1222-1313  h0 = h_prev = the initial shift; client i keeps h_i and
                                   alpha = 1 / (1 + w) in its state; step u_i = C(g - h_i),
                                   h_i += alpha u_i (cofigStep); server: u = fold, returns
                                   u + h_prev, then h_prev += alpha (S / n) u
  FRECON  algorithms.py:1056-1184  as COFIG plus g0 = g_server_prev = the gradient at x0 under the
                                   shift policy (zeros otherwise) and x_prev = x0; the client takes
                                   a second gradient at x_prev and sends q_i = C(g - g(x_prev))
                                   under the same pattern (freconStep, two messages counted per
                                   local iteration, the last q_i kept); server: q_avg +
                                   (1 - lambda_) g_server_prev + lambda_ (u + h_prev) with lambda_
                                   from the run's algorithm options, then h_prev as COFIG,
                                   x_prev = the round's starting iterate, g_server_prev = the result

The others' serverGradient bodies are covered by ``aggregation.install``.

``resident=True`` (DIANA, EF21, COFIG): the per-client state (h_i / g_i) lives in ONE
[num_clients, D] device matrix instead of in the history records, and each local iteration of a
round runs the sampled clients' steps as one call over the rows the sampling picked
(``ShiftUplinkReducer(..., clients=ids)``, the ``_sampled`` entries), with the compat patterns in
participant order.  Draw order, local steps, folds, history scalars and wire counts are those of the
default mode, and so are the iterates, bit for bit.
"""
import math
import threading

import numpy as np
import torch
import torch.nn.functional as F

from . import aggregation as ag
from . import transport


# ---------------------------------------------------------------------------------------------
# client sampling (fl_funcs.py:12-43)
# ---------------------------------------------------------------------------------------------
def get_sampled_clients(num_clients, clients_per_round, rounds, np_random, sampling="uniform", poisson_p=None):
    """All rounds' sampled clients, drawn up front from the experiment stream like the reference."""
    if sampling == "uniform":
        return [np_random.choice(num_clients, clients_per_round, replace=False) for _ in range(rounds)]
    if sampling in ("poisson", "poisson-no-empty"):
        out = []
        for _ in range(rounds):
            picked = []
            while True:
                for j in range(num_clients):
                    if np_random.uniform() < poisson_p:
                        picked.append(j)
                if picked or sampling == "poisson":
                    break
            out.append(np.asarray(picked))
        return out
    raise AssertionError("Unknown sampling type!")                         # fl_funcs.py:42


# ---------------------------------------------------------------------------------------------
# the model side: local objective of one client
# ---------------------------------------------------------------------------------------------
class DenseModel:
    """model "dense" (model_funcs.py:170-189): Flatten, Linear(d, 32), ReLU, Linear(32, 64), ReLU,
    Linear(64, out), Sigmoid, on a flat parameter vector laid out as ``model.parameters()`` is
    (mutils.get_params, mutils.py:218-255: W1, b1, W2, b2, W3, b3).  Loss: MSELoss(reduction='sum')
    (model_funcs.py:133) scaled by 1 / n_samples per batch (algorithms.py:89-90), full gradient
    over the client's data in batches of ``batch_size`` (the DataLoader, shuffle=False)."""

    def __init__(self, data, targets, samples_per_client, batch_size=32):
        self.data = torch.as_tensor(data, dtype=torch.float32)
        self.targets = torch.as_tensor(targets, dtype=torch.float32)
        self.spc = int(samples_per_client)
        self.batch_size = int(batch_size)
        d_in, d_out = self.data[0].numel(), self.targets[0].numel()
        self.shapes = [(32, d_in), (32,), (64, 32), (64,), (d_out, 64), (d_out,)]
        self.D = sum(math.prod(s) for s in self.shapes)
        self._dev = {}

    def _client_data(self, client, device):
        key = (str(device), None if client is None else int(client))
        if key not in self._dev:
            if client is None:                                  # set_client(None): the whole train set
                self._dev[key] = (self.data.to(device), self.targets.to(device))  # (artificial_dataset.py:156-158)
            else:
                lo = int(client) * self.spc
                self._dev[key] = (self.data[lo:lo + self.spc].to(device),
                                  self.targets[lo:lo + self.spc].to(device))
        return self._dev[key]

    def value_and_gradient(self, x, client):
        """(f, g): the client's loss at x as a Python float (evaluateGradient's
        function_value.item(), algorithms.py:112) and its gradient as a flat [D] fp32 tensor on
        x's device (mutils.get_gradient).  ``client=None``: the whole train set (run.py:408-413)."""
        params, off = [], 0
        for s in self.shapes:
            n = math.prod(s)
            params.append(x[off:off + n].detach().view(s).clone().requires_grad_(True))
            off += n
        data, targets = self._client_data(client, x.device)
        total = data.shape[0]
        fval = torch.zeros(1, dtype=torch.float32, device=x.device)
        grads = None
        for b0 in range(0, total, self.batch_size):
            xb = data[b0:b0 + self.batch_size].flatten(1)
            yb = targets[b0:b0 + self.batch_size]
            h = F.relu(F.linear(xb, params[0], params[1]))
            h = F.relu(F.linear(h, params[2], params[3]))
            out = torch.sigmoid(F.linear(h, params[4], params[5]))
            loss = F.mse_loss(out, yb, reduction="sum") * (1.0 / total)
            fval = fval + loss.detach()
            gb = torch.autograd.grad(loss, params)
            grads = list(gb) if grads is None else [a + b for a, b in zip(grads, gb)]   # .grad accumulation
        g = torch.cat([t.reshape(-1) for t in grads])
        return fval.item(), g


# ---------------------------------------------------------------------------------------------
# the round
# ---------------------------------------------------------------------------------------------
def l2_norm_of_vec(v):
    """mutils.l2_norm_of_vec (mutils.py:395-396): sqrt of the fp32 sum of squares, as a float."""
    return ((v ** 2).sum().item()) ** 0.5


class _Buffer:
    """The reference's Buffer contract as serverGradient consumes it (buffer.py:7-105): items in
    push order, one waitForItem() per get()."""

    def __init__(self):
        self.items = []

    def pushBack(self, item):
        self.items.append(item)

    def waitForItem(self):
        pass

    def get(self, i):
        return self.items[i]

    def __len__(self):
        return len(self.items)


def find_recent_and_remove(H, client_id, field):
    """findRecentRecordAndRemoveFromHistory (algorithms.py:371-399): the newest round that sampled
    the client holds the field (None after a previous read) or ends the search."""
    for r in sorted(H["history"], reverse=True):
        states = H["history"][r]["client_states"]
        if client_id in states:
            st = states[client_id]["client_state"]
            if field in st:
                v, st[field] = st[field], None
                return v
            return None
    return None


def _on_gpu(step):
    """Run a shift-codec client step on the MI355X whatever device the client state lives on
    (``device="cpu"``: the --gpu -1 layout, tensors cross to the GPU and back like the DCGD codec)."""
    def run(comp, *tensors, **kw):
        home = tensors[0].device
        if home.type == "cuda":
            return step(comp, *tensors, **kw)
        out = step(comp, *[t.cuda() if torch.is_tensor(t) else t for t in tensors], **kw)
        return tuple(o.to(home) for o in out) if isinstance(out, tuple) else out.to(home)
    return run


ALGORITHMS = ("dcgd", "fedavg", "diana", "ef21", "marina", "cofig", "frecon")


def parse_algorithm_options(options):
    """``--algorithm-options`` as run.py:74-79 reads it: ``"k1:v1,k2"`` -> ``{"k1": "v1", "k2": True}``
    (a dict is taken as it is)."""
    if options is None:
        return {}
    if isinstance(options, dict):
        return dict(options)
    out = {}
    for option in str(options).split(","):
        kv = option.split(":")
        if kv[0]:
            out[kv[0]] = True if len(kv) == 1 else kv[1]
    return out


class _ExperimentOptions:
    """The part of the reference's algorithms module that FRECON's serverGradient wrapper
    (aggregation.make_server_gradient_frecon) reads: the experiment-option helpers
    (algorithms.py:455-471), over ``H["experimental_options"]``."""

    @staticmethod
    def has_experiment_option(H, name):
        return name in H["experimental_options"]

    @staticmethod
    def get_experiment_option_f(H, name):
        return float(H["experimental_options"][name])


class Simulation:
    """One experiment: ``rounds`` communication rounds of ``algorithm`` (one of ``ALGORITHMS``)
    with the client codec ``client_compressor`` (the reference's spec grammar), starting at ``x0``.

    ``init_compressor`` / ``server_gradient`` / ``diana_step`` / ``ef21_step`` / ``marina_step`` /
    ``cofig_step`` / ``frecon_step`` default to the product (flpytorch_amd.aggregation: HIP codecs,
    HIP fold, fused shift codec); tests may pass other implementations of the same protocol.
    ``algorithm_options``: the run's ``--algorithm-options`` string (or a dict); FRECON reads its
    ``lambda_`` from it.  ``resident=True`` (diana, ef21, cofig; no wire modes): the module docstring's
    resident mode — same run, the clients' state rows in one device matrix, one sampled call per local
    iteration."""

    def __init__(self, algorithm, client_compressor, model, x0, num_clients, clients_per_round, rounds,
                 local_lr, global_lr, local_iters=1, runtime_seed=0, device="cuda", sampling="uniform",
                 poisson_p=None, init_compressor=None, server_gradient=None, record_iterates=False, wire=False,
                 initialize_shifts_policy="zero", diana_step=None, ef21_step=None, marina_step=None, shift_wire=False,
                 cofig_step=None, frecon_step=None, algorithm_options=None, resident=False):
        algorithm = algorithm.lower()
        if algorithm not in ALGORITHMS:
            raise ValueError(f"harness drives {', '.join(ALGORITHMS)}, not {algorithm!r}")  # algorithms.py:1954 style
        if shift_wire not in (False, True, "socket"):
            raise ValueError(f"shift_wire must be False, True or 'socket' (got {shift_wire!r})")
        if shift_wire and wire:
            raise ValueError("wire and shift_wire are separate modes: pass one of them")
        if shift_wire and algorithm not in ("diana", "ef21", "marina"):
            raise ValueError("shift_wire drives the shifted steps' messages (diana, ef21, marina) only")
        if wire and algorithm != "dcgd":
            raise ValueError("wire mode drives DCGD's compressVector messages only")
        if resident and (algorithm not in ("diana", "ef21", "cofig") or wire or shift_wire):
            raise ValueError("resident=True keeps the state rows of diana, ef21 or cofig on the device, without wire / shift_wire")
        if initialize_shifts_policy not in ("zero", "full_gradient_at_start"):
            raise ValueError(f"unknown initialize_shifts_policy {initialize_shifts_policy!r}")  # opts.py:437-441
        options = parse_algorithm_options(algorithm_options)
        if algorithm == "frecon" and "lambda_" not in options:
            # (the reference's other sources of lambda, th_stepsize_noncvx / th_stepsize_cvx, are not driven here)
            raise ValueError("frecon needs lambda_ among algorithm_options (e.g. 'lambda_:0.5')")
        self.algorithm = algorithm
        self.spec = client_compressor.lower()                                    # opts.py:497 lowercases argv
        self.model = model
        self.device = torch.device(device)
        self.x = torch.as_tensor(x0, dtype=torch.float32).reshape(-1).to(self.device).clone()
        self.D = self.x.numel()
        self.num_clients, self.per_round, self.rounds = int(num_clients), int(clients_per_round), int(rounds)
        self.local_lr, self.global_lr, self.local_iters = float(local_lr), float(global_lr), int(local_iters)
        self.record_iterates = record_iterates
        # wire=True (DCGD): each client's compressed gradient crosses the "network" as the wire
        # message (Compressor.compressPayload, include/flcodec.h layouts) and the server side
        # rebuilds it (decompressPayload, bit-exact) before the local step it applies — the
        # physical form of last_need_to_send_advance (the reference pickles dense tensors,
        # comm_socket.py:16-82); bytes per client in client_state["stats"]["payload_bytes"].
        # wire="socket": the message also crosses a real socket (transport.PayloadSocket,
        # CommSocket framing) and is checked against the codec on arrival (validatePayload)
        if wire not in (False, True, "socket"):
            raise ValueError(f"wire must be False, True or 'socket' (got {wire!r})")
        self.wire = wire
        # shift_wire=True (DIANA / EF21 / MARINA): every compressed client step ships its message
        # C(a - b) as the wire payload, written by the pass that updates the client's state
        # (Compressor.compressShiftPayload, flc_pack_shift), and the server side rebuilds the vector
        # the local step applies from it (decompressShiftPayload: m_i; g_prev + dec * mult; g_prev +
        # dec).  Uncompressed steps (EF21's first, MARINA's ck == 1) ship no payload, as without it.
        # shift_wire="socket": the payload crosses the socket pair and is validated on arrival.
        self.shift_wire = shift_wire
        self.link = transport.socket_pair() if "socket" in (wire, shift_wire) else None
        self.iterates = []                                                       # x after each round (opt-in)
        self.init_compressor = init_compressor or ag.initCompressor
        self.diana_step = diana_step or _on_gpu(ag.dianaStep)
        self.ef21_step = ef21_step or _on_gpu(ag.ef21Step)
        self.marina_step = marina_step or _on_gpu(ag.marinaStep)
        self.cofig_step = cofig_step or _on_gpu(ag.cofigStep)
        self.frecon_step = frecon_step or _on_gpu(ag.freconStep)
        # DCGD / EF21 fold then apply the master (identity) compressor (algorithms.py:1748-1770,
        # 1521-1546); FedAvg and MARINA return the fold (1810-1832, 545-563); DIANA returns h + fold
        # (1395-1421), COFIG u + h_prev (1273-1307), FRECON its combination of both folds (1124-1176)
        default_fold = {"dcgd": ag.serverGradientMaster, "ef21": ag.serverGradientMaster,
                        "fedavg": ag.serverGradientPlain, "diana": ag.serverGradientDIANA,
                        "marina": ag.serverGradientPlain, "cofig": ag.serverGradientCOFIG}.get(algorithm)
        if algorithm == "frecon" and server_gradient is None:
            default_fold = ag.make_server_gradient_frecon(_ExperimentOptions)
        self.server_gradient = server_gradient or default_fold
        self.np_random = np.random.RandomState()
        self.np_random.seed(int(runtime_seed))                                   # run.py:343-345
        self.sampled = get_sampled_clients(self.num_clients, self.per_round, self.rounds, self.np_random,
                                           sampling, poisson_p)                  # run.py:369
        master = ag.Compressor()
        master.makeIdenticalCompressor()                                         # DCGD/initializeServerState
        self.H = {"algorithm": algorithm, "D": self.D, "fl_dtype": torch.float32, "client_compressor": self.spec,
                  "compressor_master": master, "total_clients": self.num_clients, "history": {},
                  "experimental_options": options}
        if algorithm == "dcgd":
            c = self.init_compressor(self.spec, self.D)
            if c.isUnbiasedCompressor():
                self.H["w"] = c.getW()
            elif c.isContractionCompressor():
                self.H["alpha"] = c.getAlphaContraction()
        elif algorithm == "diana":                                               # algorithms.py:1346-1357
            w = self.init_compressor(self.spec, self.D).getW()
            if initialize_shifts_policy == "full_gradient_at_start":             # run.py:408-413
                _, h0 = self.model.value_and_gradient(self.x, None)
            else:
                h0 = torch.zeros(self.D, dtype=torch.float32, device=self.device)
            self.H.update({"h0": h0.detach().clone(), "h": h0.detach().clone(), "alpha": 1.0 / (1.0 + w), "w": w})
        elif algorithm == "ef21":                                                # algorithms.py:1460-1468
            self.H["request_use_full_list_of_clients"] = True
        elif algorithm == "marina":                                              # algorithms.py:486-492
            # test_ber_rv = 0 forces a full-gradient first round
            self.H.update({"x_prev": self.x.clone(), "test_ber_rv": 0.0})
        elif algorithm in ("cofig", "frecon"):                                   # algorithms.py:1222-1233, 1056-1067
            if initialize_shifts_policy == "full_gradient_at_start":             # run.py:408-417
                _, grad_start = self.model.value_and_gradient(self.x, None)
            else:
                grad_start = torch.zeros(self.D, dtype=torch.float32, device=self.device)
            grad_start = grad_start.detach()
            self.H.update({"h0": grad_start.clone(), "h_prev": grad_start.clone()})   # (zero policy: zeros, 474-479)
            if algorithm == "frecon":
                self.H.update({"g0": grad_start.clone(), "g_server_prev": grad_start.clone(),
                               "x_prev": self.x.clone()})
        # resident=True: row c of `state` is client c's h_i (DIANA / COFIG: h0 until its first step) or
        # g_i (EF21: no row until its first, uncompressed step: state_set[c])
        self.resident = bool(resident)
        if self.resident:
            gpu = self.device if self.device.type == "cuda" else torch.device("cuda")
            self.state = torch.zeros((self.num_clients, self.D), dtype=torch.float32, device=gpu)
            self.state_set = [algorithm != "ef21"] * self.num_clients
            if algorithm != "ef21":
                self.state.copy_(self.H["h0"].to(gpu).unsqueeze(0).expand_as(self.state))
            self.uplink = ag.ShiftUplinkReducer(ag.initCompressor(self.spec, self.D), device=gpu)

    # algorithms.clientState (2015-2069) with the class parts: DCGD 1729-1732, FedAvg 1793-1794,
    # DIANA 1360-1373, EF21 1471-1484, MARINA 495-509, COFIG 1236-1249, FRECON 1070-1089
    def client_state(self, client_id, rnd):
        cs = {}
        if self.algorithm in ("dcgd", "diana", "ef21", "marina", "cofig", "frecon"):
            comp = self.init_compressor(self.H["client_compressor"], self.D)
            comp.generateCompressPattern(self.np_random, str(self.device), client_id, self.H)
            cs["client_compressor"] = comp
        if self.algorithm == "marina":
            p = 1.0 / (1.0 + comp.getW())
            cs.update({"p": p, "ck": 1 if self.H["test_ber_rv"] <= p else 0})
        if self.algorithm in ("diana", "cofig", "frecon"):
            if not self.resident:                                                # (resident: row client_id of self.state)
                hi = find_recent_and_remove(self.H, client_id, "hi")
                cs["hi"] = self.H["h0"].detach().clone() if hi is None else hi
            if self.algorithm != "diana":
                cs["alpha"] = 1.0 / (1.0 + comp.getW())
        elif self.algorithm == "ef21" and not self.resident:
            cs["g_prev"] = find_recent_and_remove(self.H, client_id, "g_prev")
        cs.update({"algorithm": self.algorithm, "client_id": client_id, "weight": 1.0, "round": rnd,
                   "approximate_f_value": [], "seed": self.np_random.randint(2 ** 31),
                   "stats": {"send_scalars_to_master": 0}})
        return cs

    # the class's localGradientEvaluation after the gradient is known: the vector the local SGD
    # step applies
    def client_step(self, cs, g):
        comp = cs.get("client_compressor")
        if self.algorithm == "fedavg":                                           # algorithms.py:1803-1807
            cs["stats"]["send_scalars_to_master"] += g.numel()
            return g
        if self.algorithm == "dcgd":                                             # algorithms.py:1741-1745
            if self.wire:
                msg = comp.compressPayload(g)
                cs["stats"]["payload_bytes"] = cs["stats"].get("payload_bytes", 0) + msg.numel()
                if self.link is not None:
                    msg = self.transfer(comp, msg, g.numel())
                c = comp.decompressPayload(msg, g.numel())
            else:
                c = comp.compressVector(g)
            cs["stats"]["send_scalars_to_master"] += comp.last_need_to_send_advance
            return c
        if self.shift_wire:
            return self.client_step_shift_wire(cs, comp, g)
        if self.algorithm == "diana":                                            # algorithms.py:1383-1392
            m, cs["hi"] = self.diana_step(comp, g, cs["hi"], self.H["alpha"])
            cs["stats"]["send_scalars_to_master"] += comp.last_need_to_send_advance
            return m
        if self.algorithm == "cofig":                                            # algorithms.py:1265-1270
            u, cs["hi"] = self.cofig_step(comp, g, cs["hi"], cs["alpha"])
            cs["stats"]["send_scalars_to_master"] += comp.last_need_to_send_advance
            return u
        if self.algorithm == "frecon":                                           # algorithms.py:1103-1121
            # the gradient at the server's previous iterate (its function value is not recorded), then
            # both messages under the one pattern; each counts on the wire, the local step applies u_i
            _, g_old = self.model.value_and_gradient(self.H["x_prev"], cs["client_id"])
            u, cs["hi"], cs["qi"] = self.frecon_step(comp, g, cs["hi"], g_old, cs["alpha"])
            cs["stats"]["send_scalars_to_master"] += 2 * comp.last_need_to_send_advance
            return u
        if self.algorithm == "marina":                                           # algorithms.py:512-540
            if cs["ck"] == 1:
                cs["stats"]["send_scalars_to_master"] += g.numel()
                return g
            # the gradient at the previous iterate (its function value is not recorded), then
            # g_prev + C(grad_cur - grad_prev) in one fused pass
            _, g_old = self.model.value_and_gradient(self.H["x_prev"], cs["client_id"])
            g_next = self.marina_step(comp, g, g_old, self.H["g_prev"].to(g.device))
            cs["stats"]["send_scalars_to_master"] += comp.last_need_to_send_advance
            return g_next
        if cs["g_prev"] is None:                                                 # EF21, algorithms.py:1494-1500
            cs["g_prev"] = g                                                     # (first step: not counted)
            return g
        g_next = self.ef21_step(comp, g, cs["g_prev"])                           # algorithms.py:1502-1518
        cs["stats"]["send_scalars_to_master"] += comp.last_need_to_send_advance
        cs["g_prev"] = g_next
        return g_next

    def client_step_shift_wire(self, cs, comp, g):
        """client_step's DIANA / EF21 / MARINA branches with the message on the wire: the client
        half is one compressShiftPayload call, the server half one decompressShiftPayload call whose
        result — bit for bit the plain step's — is what the local step applies."""
        home, d = g.device, g.numel()

        # the product's codec runs on the MI355X whatever device the client state lives on (like
        # _on_gpu); another implementation of the protocol (a test's double) takes the tensors as they are
        on_gpu = isinstance(comp, ag.Compressor)

        def dev(t):
            return t.cuda() if on_gpu and t.device.type != "cuda" else t

        def ship(payload):
            cs["stats"]["payload_bytes"] = cs["stats"].get("payload_bytes", 0) + payload.numel()
            return self.transfer(comp, payload, d) if self.link is not None else payload
        if self.algorithm == "diana":                                            # algorithms.py:1383-1392
            h = dev(cs["hi"])
            payload, _, h_new = comp.compressShiftPayload(dev(g), h, alpha=self.H["alpha"], shift=h)
            cs["hi"] = h_new.to(home)
            out = comp.decompressShiftPayload(ship(payload), d)
        elif self.algorithm == "marina":                                         # algorithms.py:512-540
            if cs["ck"] == 1:
                cs["stats"]["send_scalars_to_master"] += d
                return g
            _, g_old = self.model.value_and_gradient(self.H["x_prev"], cs["client_id"])
            payload, _, _ = comp.compressShiftPayload(dev(g), dev(g_old))
            out = comp.decompressShiftPayload(ship(payload), d, base=dev(self.H["g_prev"].to(home)))
        else:                                                                    # EF21, algorithms.py:1494-1518
            if cs["g_prev"] is None:
                cs["g_prev"] = g                                                 # (first step: not counted)
                return g
            mult = 1.0 if comp.isContractionCompressor() else 1.0 / (1.0 + comp.getW())
            g_prev = dev(cs["g_prev"])
            payload, g_next, _ = comp.compressShiftPayload(dev(g), g_prev, scale=mult, base=g_prev, message=True)
            cs["g_prev"] = g_next.to(home)                                       # the client's own estimator
            out = comp.decompressShiftPayload(ship(payload), d, scale=mult, base=g_prev)   # the server's mirror
        cs["stats"]["send_scalars_to_master"] += comp.last_need_to_send_advance
        return out.to(home)

    def transfer(self, comp, msg, d):
        """One message client -> server over the socket pair: the client end sends on a thread
        (a message larger than the socket buffer would otherwise block), the server end receives
        and validates it; returns the received host uint8 tensor."""
        client, server = self.link
        err = []

        def send():
            try:
                client.sendPayload(msg)
            except Exception as e:                      # surfaced after the join
                err.append(e)
        t = threading.Thread(target=send, daemon=True)
        t.start()
        try:
            got = server.recvPayload(comp, d)
        except BaseException:
            # a refused or broken message: unblock the sender (it may sit in sendall on a full
            # socket buffer) before waiting for it
            server.abort()
            client.abort()
            t.join(timeout=30)
            raise
        t.join()
        if err:
            raise err[0]
        return got

    # local_training (model_funcs.py:318-388) + train_model's loop (617-723)
    def local_training(self, cs, client_id):
        xi = self.x.clone()
        for _ in range(self.local_iters):
            f, g = self.model.value_and_gradient(xi, client_id)
            c = self.client_step(cs, g)
            cs["approximate_f_value"].append(f)
            xi.add_(c.to(xi.device), alpha=-self.local_lr)                      # SGD step, momentum 0
        return {"model": xi, "client_id": client_id, "client_state": cs}

    # resident=True: the sampled clients of a round in lockstep.  clientState draws (pattern, seed)
    # per client in the reference's order first: local training draws nothing from the stream
    def resident_training(self, clients, rnd):
        ids = [int(c) for c in clients]
        states = [self.client_state(cid, rnd) for cid in ids]
        xs = [self.x.clone() for _ in ids]
        for _ in range(self.local_iters if ids else 0):
            fg = [self.model.value_and_gradient(xi, cid) for xi, cid in zip(xs, ids)]
            G = torch.stack([g.to(self.state.device) for _, g in fg])
            C = self.resident_step(states, ids, G)
            for xi, cs, (f, _), c in zip(xs, states, fg, C):
                cs["approximate_f_value"].append(f)
                xi.add_(c.to(xi.device), alpha=-self.local_lr)                  # SGD step, momentum 0
        return [{"model": xi, "client_id": cid, "client_state": cs} for xi, cid, cs in zip(xs, ids, states)]

    def resident_patterns(self, comps):
        """The clients' compat patterns as the rows of one call, in participant order."""
        t, dev = comps[0].compressorType, self.state.device
        if t == ag.CompressorType.RANDK_COMPRESSOR:
            return {"randk_idx": torch.stack([c.S.to(device=dev, dtype=torch.int64) for c in comps])}
        if t in (ag.CompressorType.NATURAL_COMPRESSOR_FP32, ag.CompressorType.STANDARD_DITHERING_FP32,
                 ag.CompressorType.NATURAL_DITHERING_FP32):
            return {"uniforms": torch.stack([c.testp.to(device=dev) for c in comps])}
        if t == ag.CompressorType.LAZY_COMPRESSOR:
            return {"lazy_u": torch.tensor([c.testp for c in comps], dtype=torch.float64, device=dev)}
        return {}

    def resident_step(self, states, ids, G):
        """client_step for every sampled client at once: G [n, D] the local gradients, the result
        [n, D] the vectors their local steps apply; the state rows ids are updated in place."""
        if self.algorithm == "ef21":                                             # algorithms.py:1494-1518
            C = torch.empty_like(G)
            have = [i for i, cid in enumerate(ids) if self.state_set[cid]]
            for i, cid in enumerate(ids):
                if not self.state_set[cid]:                                      # (first step: not counted)
                    self.state[cid].copy_(G[i])
                    self.state_set[cid] = True
                    C[i].copy_(G[i])
            if not have:
                return C
            comps = [states[i]["client_compressor"] for i in have]
            sub = [ids[i] for i in have]
            mult = 1.0 if comps[0].isContractionCompressor() else 1.0 / (1.0 + comps[0].getW())
            self.uplink(G if len(have) == len(ids) else G[have], self.state, scale=mult, base=self.state,
                        msg_out=self.state, clients=sub, **self.resident_patterns(comps))
            C[have] = self.state[sub]
        else:                                                                    # algorithms.py:1383-1392, 1265-1270
            have = list(range(len(ids)))
            comps = [cs["client_compressor"] for cs in states]
            alpha = self.H["alpha"] if self.algorithm == "diana" else states[0]["alpha"]
            C = torch.empty_like(G)
            self.uplink(G, self.state, alpha=alpha, shift=self.state, shift_out=self.state, msg_out=C, clients=ids,
                        indexed=("b", "shift", "shift_out"), **self.resident_patterns(comps))
        for i, comp in zip(have, comps):                                         # each client's own wire count
            comp._account(self.D)
            states[i]["stats"]["send_scalars_to_master"] += comp.last_need_to_send_advance
        return C

    # run_one_communication_round (model_funcs.py:459-614)
    def run_round(self, rnd):
        if self.H.get("request_use_full_list_of_clients"):                       # model_funcs.py:470-475
            clients = np.arange(self.H["total_clients"])
        else:
            clients = self.sampled[rnd]
        buf = _Buffer()
        if self.resident:
            for item in self.resident_training(clients, rnd):
                buf.pushBack(item)
        else:
            for cid in clients:
                cs = self.client_state(int(cid), rnd)
                buf.pushBack(self.local_training(cs, int(cid)))
        n = len(clients)
        x_prev = self.x.clone()
        if n == 0:
            gs = torch.zeros_like(self.x)                                        # algorithms.py:2117-2118
        else:
            gs = self.server_gradient(buf, n, None, x_prev, self.H)
        self.x.add_(gs, alpha=-self.global_lr)                                   # global SGD step
        if self.record_iterates:
            self.iterates.append(self.x.detach().cpu().clone())
        fvalues = []
        states = {}
        for item in buf.items:
            fvalues += item["client_state"]["approximate_f_value"]
            st = item["client_state"]
            st.pop("client_compressor", None)                                    # algorithms.py:2198-2199
            states[item["client_id"]] = {"client_state": st}
        self.H["history"][rnd] = {
            "client_states": states,
            "grad_sgd_server_l2": l2_norm_of_vec(gs),
            "approximate_f_avg_value": float(np.mean(fvalues)) if fvalues else float("nan"),
            "x_before_round": l2_norm_of_vec(x_prev),
        }
        # the class's serverGlobalStateUpdate (2239-2240)
        if self.algorithm == "diana":                                            # algorithms.py:1424-1428
            self.H["h"] = self.H["h"] + self.H["alpha"] * self.H["m"]
        elif self.algorithm == "ef21":                                           # algorithms.py:1549-1554
            self.H["compressor_master"].generateCompressPattern(self.np_random, str(self.device), -1, self.H)
            self.H["request_use_full_list_of_clients"] = False
        elif self.algorithm in ("cofig", "frecon") and "alpha_update" in self.H:  # algorithms.py:1309-1313, 1179-1184
            self.H["h_prev"] = self.H["h_prev"] + self.H["alpha_update"] * self.H["u_avg_update"]
            if self.algorithm == "frecon":
                self.H["x_prev"] = x_prev
                self.H["g_server_prev"] = gs
        elif self.algorithm == "marina":                                         # algorithms.py:566-572
            self.H["g_prev"] = gs
            self.H["x_prev"] = self.x.clone()                                    # the iterate after the step
            self.H["test_ber_rv"] = self.np_random.random()
        return self.H["history"][rnd]

    def run(self):
        for r in range(self.rounds):
            prev = self.H["history"].get(r - 1)
            if prev is not None and any(math.isnan(prev[k]) or math.isinf(prev[k])
                                        for k in ("x_before_round", "grad_sgd_server_l2")):
                break                                                            # run.py:466-479
            self.run_round(r)
        return self.H
