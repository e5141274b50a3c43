"""``Attacker`` -- the reference's attack driver (attacker.py:14-417) on the HIP probe primitive.

Same constructor, method names, prints and result file as the reference, so
``GCNTrainer.eval_output`` (gcn_trainer.py:320-339) can use it unchanged.  What differs is how
``influence_val`` is produced: instead of ``n_test`` pairs of full forwards and ``n_test**2``
``.norm().item()`` host syncs (attacker.py:220-229), one call to ``lt_influence_rows`` fills this
rank's rows on the device and a single copy brings the matrix back.

Extra, optional ``args`` fields (absent in the reference's namespace -> defaults):
    influence_mode   'delta' (default: the perturbation propagated exactly; AUC / AP equal the reference evaluated
                     in fp64) | 'sparse' (the reference's fp32 finite difference, bit-identical to 'full') | 'full'
"""
from __future__ import annotations

import os
import os.path as osp
import time

import numpy as np
import torch
from sklearn import metrics

from . import dist as lt_dist
from . import engine
from ._lib import LinkTellerHipError
from .sampling import construct_balanced_edge_sets, construct_edge_sets_from_random_subgraph

# args.baseline_scores / --baseline-scores: the values that form the baseline attacks' scores on the GPU, and those of them that
# also admit the chunked recovery from the command line (main.check_*, GCNTrainer and Attacker._baseline_route all read these)
DEVICE_BASELINE_SCORES = ("device", "stream")
STREAM_BASELINE_SCORES = ("stream",)


class Attacker:
    def __init__(self, args, model, worker):
        self.args = args
        self.dataset = args.dataset
        self.model = model
        self.worker = worker

        if args.sample_type == "balanced-full":
            self.args.n_test = self.worker.n_nodes           # attacker.py:21-22

        if self.dataset.startswith("twitch") or self.dataset.startswith("deezer"):
            self.features = self.worker.features_2           # attacker.py:24-26
            self.adj = self.worker.adj_2
        else:
            self.features = self.worker.features             # attacker.py:28-30
            self.adj = self.worker.adj_full
        self._baseline = None
        self._baseline_key = None
        self.influence_val = None

    # ------------------------------------------------------------------------------------------
    def prepare_test_data(self, pairs="host", rng="numpy"):
        """attacker.py:33-48.  'balanced' and 'bfs' cannot run in the reference either (tuple
        arity / signature mismatches at attacker.py:46-47); 'balanced-full' can.

        ``pairs="device"`` / ``rng="philox"`` (additions; the defaults are the reference's host route) keep the pairs on the GPU:
          * ``unbalanced*`` with ``pairs="device"``: the nodes are drawn as on the host route (the same ``np.random`` stream, the
            same sample); their pairs are never enumerated on the host.  ``evaluate`` (efficient attack) reads labels and index
            from ``sampling.square_labels_device``, built on first use; ``recover_edges`` takes the edge count and ``is_edge``
            from the label triangle.
          * ``balanced-full`` with ``rng="philox"`` (implies device pairs): edges and non-edges come from
            ``sampling.balanced_pairs_philox`` -- Philox stream 3, DIFFERENT non-edges than numpy's stream gives for the seed --
            and stay on the device; ``evaluate`` groups them with ``engine.group_pairs_device`` and scores them with
            ``Baseline.influence_pairs``.  ``balanced-full`` with ``pairs="device"`` and ``rng="numpy"`` is the host route: the
            numpy stream is a host loop.
          * ``rng="philox"`` with an ``unbalanced*`` type is a ``ValueError``: its node draw stays on numpy.
        Both need a GPU (``LinkTellerHipError`` without one).  Whatever the device routes do not serve -- the attack methods that
        write a result file, the naive and baseline attacks on an ``unbalanced*`` sample, a model without a pair-list
        primitive (``_pair_route``: none of ``engine.Baseline``, ``engine.Baseline2W`` and ``engine.Baseline3`` serves it), CPU features -- FALLS BACK to the host lists: ``exist_edges`` / ``nonexist_edges`` are
        materialised from one download on first access (the arrays the host route builds, element for element, for the
        ``unbalanced*`` types) and everything proceeds as on the host route, raising what it raises there."""
        st = self.args.sample_type
        if pairs not in ("host", "device"):
            raise ValueError(f"pairs = {pairs!r}: 'host' or 'device'")
        if rng not in ("numpy", "philox"):
            raise ValueError(f"rng = {rng!r}: 'numpy' or 'philox'")
        if rng == "philox" and st != "balanced-full":
            raise ValueError(f"rng = 'philox' serves sample_type = balanced-full only (got {st}: its nodes are drawn from numpy's stream)")
        self._sample_dev = None
        if rng == "philox" or (pairs == "device" and str(st).startswith("unbalanced")):
            return self._prepare_on_device(st)
        func = {"unbalanced": construct_edge_sets_from_random_subgraph,
                "unbalanced-lo": construct_edge_sets_from_random_subgraph,
                "unbalanced-hi": construct_edge_sets_from_random_subgraph,
                "balanced-full": construct_balanced_edge_sets}.get(st)
        if not func:
            raise NotImplementedError(f"sample_type = {st} not implemented!")
        np.random.seed(self.args.sample_seed)
        (self.exist_edges, self.nonexist_edges), self.test_nodes = func(
            self.dataset, st, self.worker.adj_ori, self.args.n_test)
        print("generating testing (non-)edge set done!")

    # ---- the pairs on the device ------------------------------------------------------------------------
    def _pattern_csr(self):
        """The structural pattern of ``worker.adj_ori`` on the device, uploaded once per adjacency object."""
        from . import sampling
        c = getattr(self, "_pattern_cache", None)
        if c is None or c[0] is not self.worker.adj_ori:
            c = self._pattern_cache = (self.worker.adj_ori, sampling.device_pattern_csr(self.worker.adj_ori))
        return c[1]

    def _prepare_on_device(self, st):
        import scipy.sparse as sp
        from . import _lib, sampling
        _lib.require_gpu()
        csr = self._pattern_csr()
        self.__dict__.pop("_exist_edges", None)
        self.__dict__.pop("_nonexist_edges", None)
        if st == "balanced-full":
            u, v, n_edges, info = sampling.balanced_pairs_philox(csr, self.args.sample_seed)
            self.test_nodes = list(range(self.worker.n_nodes))
            self._sample_dev = {"kind": "balanced", "u": u, "v": v, "n_edges": n_edges, "info": info}
            print(f"sampling done! len(edge_set) = {n_edges}, len(nonedge_set) = {n_edges}")
        else:
            np.random.seed(self.args.sample_seed)
            nodes = sampling.draw_subgraph_nodes(self.dataset, st, sp.csr_matrix(self.worker.adj_ori), self.args.n_test)
            print("#nodes =", len(nodes))
            self.test_nodes = nodes
            self._sample_dev = {"kind": "square", "lists": {}, "n_edges": None}
        print("generating testing (non-)edge set done!")

    def _square_lists(self, lds, dev):
        """(index, labels, info) of the sampled square on the device for score rows of stride ``lds``: built on first use, kept
        per stride (the labels of the first build serve every stride)."""
        from . import sampling
        d = self._sample_dev
        hit = d["lists"].get((lds, dev))
        if hit is None:
            probes, _ = self._device_nodes(np.asarray(self.test_nodes, dtype=np.int64), 0, len(self.test_nodes))
            hit = d["lists"][(lds, dev)] = sampling.square_labels_device(self._pattern_csr(), probes, lds)
        return hit

    def _square_n_edges(self, info):
        """The sample's edge count (and the device's check of the node list) from an info block: one copy of 4 words, once."""
        from . import sampling
        d = self._sample_dev
        if d["n_edges"] is None:
            d["n_edges"] = sampling.check_square_info(info)
        return d["n_edges"]

    def _materialise_pairs(self):
        """The host lists of a device-prepared sample, from ONE download (the label triangle / the two pair arrays)."""
        from . import sampling
        d = self._sample_dev
        if d["kind"] == "square":
            nodes = np.asarray(self.test_nodes, dtype=np.int64)
            k = len(nodes)
            if d["lists"]:
                _, labels, info = next(iter(d["lists"].values()))
            else:
                _, labels, info = sampling.square_labels_device(self._pattern_csr(), nodes, k, index=False)
            self._square_n_edges(info)
            present = labels.cpu().numpy() != 0
            iu, ju = np.triu_indices(k, k=1)
            pairs = np.stack([nodes[iu], nodes[ju]], axis=1)
            ex, nex = pairs[present], pairs[~present]
            print("#edges_set =", len(ex))
            print("#nonedge_set =", len(nex))
        else:
            e = d["n_edges"]
            uv = np.stack([d["u"].cpu().numpy().astype(np.int64), d["v"].cpu().numpy().astype(np.int64)], axis=1)
            ex, nex = uv[:e], uv[e:]
        self.__dict__["_exist_edges"], self.__dict__["_nonexist_edges"] = ex, nex

    def _host_list(self, name):
        if name not in self.__dict__:
            if getattr(self, "_sample_dev", None) is None:
                raise AttributeError(f"'Attacker' object has no attribute '{name[1:]}'")
            self._materialise_pairs()
        return self.__dict__[name]

    exist_edges = property(lambda self: self._host_list("_exist_edges"),
                           lambda self, value: self.__dict__.__setitem__("_exist_edges", value))
    nonexist_edges = property(lambda self: self._host_list("_nonexist_edges"),
                              lambda self, value: self.__dict__.__setitem__("_nonexist_edges", value))

    # ------------------------------------------------------------------------------------------
    _TWO = ("gc1.weight", "gc1.bias", "gc2.weight", "gc2.bias")
    _THREE = _TWO + ("gc3.weight", "gc3.bias")

    def _walk(self):
        """ONE ``state_dict()`` walk per attack (it costs ~10 us per call on a 2-layer module; the round-4 path made three):
        (kind, state_dict) with kind 'gcn2' | 'gcn3' | 'gcn3w' (within what lt_baseline3 serves: up to 8 classes, 9 .. 256
        classes) | 'generic'."""
        # (and that one walk is skipped while the model's parameters are the very objects -- and storages -- of the last walk: four
        # attribute reads instead of ~10 us of state_dict(); a load_state_dict() copies in place and is seen by the baseline's
        # refresh, a replaced parameter / a moved module changes the identity or the data pointer and walks again)
        c = getattr(self, "_walk_cache", None)
        if c is not None:
            try:
                if c[0] is self.model:
                    ok = True
                    for g, p, q, parent, child, owner, name in c[1]:
                        # (two dict look-ups instead of nn.Module.__getattr__ twice: "gc1.weight" is model._modules["gc1"]._parameters["weight"])
                        if owner is not None:
                            if parent._modules.get(child) is not owner or owner._parameters.get(name) is not p or p.data_ptr() != q:
                                ok = False
                                break
                        elif g(self.model) is not p or p.data_ptr() != q:
                            ok = False
                            break
                    if ok:
                        return c[2], c[3]
            except AttributeError:
                pass
        sd = self.model.state_dict()
        keys = sd.keys()
        if len(keys) == 4 and all(k in sd for k in self._TWO):
            kind = "gcn2"
        elif (len(keys) == 6 and all(k in sd for k in self._THREE) and sd["gc1.weight"].shape[1] <= 256
                and sd["gc2.weight"].shape[1] <= 256 and sd["gc3.weight"].shape[1] <= 256):
            # GCN3 (gcn/models.py:28-46): hidden widths <= 256; <= 8 classes, or the wide class layer (reddit 41, ppi 121)
            kind = "gcn3" if sd["gc3.weight"].shape[1] <= 8 else "gcn3w"
        else:
            kind = "generic"
        self._walk_cache = None
        try:
            import operator
            trip = []
            for k in keys:
                g = operator.attrgetter(k)
                prm = g(self.model)
                if not isinstance(prm, torch.Tensor) or prm.data_ptr() != sd[k].data_ptr():
                    raise AttributeError(k)
                parts = k.split(".")
                parent = child = owner = name = None
                if len(parts) == 2 and self.model._modules.get(parts[0]) is not None and \
                        self.model._modules[parts[0]]._parameters.get(parts[1]) is prm:
                    parent, child, owner, name = self.model, parts[0], self.model._modules[parts[0]], parts[1]
                trip.append((g, prm, prm.data_ptr(), parent, child, owner, name))
            self._walk_cache = (self.model, trip, kind, sd)
        except AttributeError:
            pass                   # (a model whose state_dict keys are not attribute paths: walk every time)
        return kind, sd

    def _params(self, sd=None):
        sd = self.model.state_dict() if sd is None else sd
        try:
            return [sd[k].detach() for k in self._TWO]
        except KeyError as e:
            raise NotImplementedError(f"the probe kernels need a 2-layer GCN state_dict (missing {e})") from None

    def _is_two_layer(self):
        return self._walk()[0] == "gcn2"

    def _layers(self, sd=None):
        """[(W, b), ...] of a GraphConvolution stack (gc1, gc2, gc3, ...), on the features' device."""
        sd, out, i = (self.model.state_dict() if sd is None else sd), [], 1
        while f"gc{i}.weight" in sd:
            out.append((sd[f"gc{i}.weight"].detach().to(self.features.device),
                        sd[f"gc{i}.bias"].detach().to(self.features.device)))
            i += 1
        if not out:
            raise NotImplementedError("model has no gc<i>.weight layers")
        return out

    def _rows_generic(self, probe_nodes, observe_nodes, sd=None):
        """Probe rows for GraphConvolution stacks neither probe primitive covers (more than 3 layers, a GCN3 wider than
        256 hidden units or classes, and `sparse` / `full` of a GCN3 with 9 .. 256 classes): per probe, row v of S1 = X W1 is replaced by (x_v + x_v*d) W1 and
        the remaining layers run through lt_spmm_csr_f32 / lt_gemm_f32.  Same quantity, ~2 launches per layer per
        probe; kept as the reference implementation the 3-layer primitive is tested against."""
        layers = self._layers(sd)
        x, delta = self.features, float(self.args.influence)
        g = engine.as_hip_graph(self.adj)

        def rest(s1):
            h = engine.spmm(g, s1, layers[0][1], relu=len(layers) > 1)
            for li, (w, b) in enumerate(layers[1:], start=1):
                h = engine.spmm(g, engine.gemm(h, w), b, relu=li < len(layers) - 1)
            return h

        def ids(nodes, what):
            # node lists arrive as numpy / lists (direct callers) or as the cached int32 device lists of _device_nodes
            # (influence_matrix); out-of-range ids raise IndexError as the reference's features[v] does (attacker.py:103)
            if isinstance(nodes, torch.Tensor):
                t = nodes.to(device=x.device, dtype=torch.long)
            else:
                t = torch.as_tensor(np.asarray(nodes, dtype=np.int64), device=x.device)
            if t.numel() and (int(t.min()) < 0 or int(t.max()) >= int(x.shape[0])):
                raise IndexError(f"{what}: node id out of range for {int(x.shape[0])} nodes")
            return t

        s1 = engine.gemm(x, layers[0][0])
        obs = ids(observe_nodes, "observe_nodes")
        probe_ids = ids(probe_nodes, "probe_nodes").tolist()
        base = rest(s1)[obs]
        rows = torch.empty((len(probe_ids), obs.numel()), dtype=torch.float32, device=x.device)
        for i, v in enumerate(probe_ids):
            xv = x[v]
            s1p = s1.clone()
            s1p[v] = engine.gemm((xv + xv * delta)[None, :].contiguous(), layers[0][0])[0]
            rows[i] = ((rest(s1p)[obs] - base) / delta).norm(dim=1)
        return rows

    def _is_three_layer(self):
        return self._walk()[0] == "gcn3"

    def baseline3(self, sd=None) -> engine.Baseline3:
        """The 3-layer counterpart of ``baseline()``: same caching rule (rebuilt when features / adjacency /
        parameters were replaced, refreshed on every attack)."""
        dev = self.features.device
        sd = self.model.state_dict() if sd is None else sd
        src = [sd[f"gc{i}.{p}"].detach() for i in (1, 2, 3) for p in ("weight", "bias")]
        off_device = any(p.device != dev for p in src)
        key = ("gcn3", id(self.adj), self.features.data_ptr(),
               tuple((p.data_ptr(), p._version if off_device else 0) for p in src))
        if self._baseline is None or self._baseline_key != key:
            self._baseline = engine.Baseline3(self.adj, self.features, *[p.to(dev) for p in src])
            self._baseline_key = key
        else:
            self._baseline.refresh()
        return self._baseline

    def _mode(self, mode=None):
        return mode or getattr(self.args, "influence_mode", None) or os.environ.get("LT_INFLUENCE_MODE", "delta")

    def _rows(self, probe_nodes, observe_nodes, mode=None):
        """[len(probe_nodes), len(observe_nodes)] influence rows on the device."""
        kind, sd = self._walk()
        if kind == "gcn2":
            mode = self._mode(mode)
            # (beyond 8 classes: engine.Baseline2W in `delta`; engine.WideBaseline, slice by slice, for every other mode and beyond
            # 256 hidden units)
            base = self.baseline(mode, sd)
            return base.influence_rows(probe_nodes, observe_nodes, float(self.args.influence), mode)
        if kind == "gcn3":
            # the 3-hop probe primitive: `delta` (default) propagates the perturbation exactly through the three layers,
            # `sparse` / `full` are the reference's fp32 finite difference on the rows a probe can reach
            return self.baseline3(sd).influence_rows(probe_nodes, observe_nodes, float(self.args.influence), self._mode(mode))
        if kind == "gcn3w" and self._mode(mode) == "delta":
            # 9 .. 256 classes: `delta` through the wide handle (lt_baseline3_create_wide); `sparse` / `full` stay the loop below
            return self.baseline3(sd).influence_rows(probe_nodes, observe_nodes, float(self.args.influence), "delta")
        return self._rows_generic(probe_nodes, observe_nodes, sd)

    def _device_nodes(self, nodes, b, e):
        """(this rank's probes, all observed nodes) as int32 device lists, validated on the host ONCE per distinct node list
        (the round-4 path re-validated and re-uploaded both lists on every attack); the key is the list's content."""
        dev = self.features.device
        if dev.type != "cuda":
            return nodes[b:e], nodes            # (engine refuses CPU tensors with its own message)
        key = (nodes.tobytes(), dev.index)
        hit = getattr(self, "_node_cache", None)
        if hit is None or hit[0] != key:
            obs = engine._as_nodes(nodes, int(self.features.shape[0]), dev, "test_nodes")
            hit = self._node_cache = (key, {}, obs)
        sl = hit[1].get((b, e))
        if sl is None:                          # (a contiguous slice of a 1-d tensor: a view, no copy)
            sl = hit[1][(b, e)] = hit[2] if (b, e) == (0, len(nodes)) else hit[2][b:e]
        return sl, hit[2]

    def baseline(self, mode=None, sd=None) -> engine.Baseline:
        """Loop-invariant model(features, adj) of attacker.py:106: built once per (features, adj, parameters) --
        rebuilt when any of them was replaced, refreshed (X W1 recomputed from the borrowed tensors) on every attack
        so that in-place weight updates are seen.  In-place torch edits of the features are seen too (the refresh compares the
        tensor's version counter and has the baseline's difference lists of X rebuilt); features written behind torch's back
        -- through a raw pointer -- are announced with ``baseline().features_changed()``.  With several ranks the product the MODE reads (fp32 X W1 for `full` /
        `sparse`, the fp64 one for `delta`) is sharded or replicated per ``dist.choose_baseline_sharding``."""
        mode = self._mode(mode)
        # A class layer of 9 .. 256 columns behind a hidden layer of up to 256 (engine.wide_class_shapes) has two routes: the ONE
        # handle of engine.Baseline2W, which serves `delta` alone, and the slices of engine.WideBaseline (every mode; LT_WIDE2=slices
        # keeps it in `delta` too, with its bits).  The handle is the default: profiles/wide2_attack_time.json.  Which of the two
        # a mode wants is part of the cache key: a switch between `delta` and `sparse` / `full` on such a model rebuilds.
        want2w = mode == "delta" and os.environ.get("LT_WIDE2", "handle") != "slices"
        # (the very state_dict of the last call -- _walk() hands the same object back while no parameter was replaced or moved --
        # with the same adjacency and feature storage: the key below would come out the same; ~4 us of Python in front of the first
        # launch of every attack.  Parameters on another device are copies: their in-place updates need the full check.)
        same = getattr(self, "_key_same", None)
        if (sd is not None and same is not None and self._baseline is not None and same[0] is sd and same[1] is self.adj
                and same[2] is self.features and same[3] == self.features.data_ptr() and same[4] == want2w):
            created = False
        else:
            dev = self.features.device
            src = self._params(sd)
            off_device = any(p.device != dev for p in src)
            use2w = want2w and engine.wide_class_shapes(src[0].shape[1], src[2].shape[1])
            # parameters held on another device are copied: then an in-place update (p._version) means a rebuild too
            key = (id(self.adj), self.features.data_ptr(), tuple((p.data_ptr(), p._version if off_device else 0) for p in src), use2w)
            created = self._baseline is None or self._baseline_key != key
            if created:
                make = engine.Baseline2W if use2w else engine.baseline_for
                self._baseline = make(self.adj, self.features, *[p.to(dev) for p in src])
                self._baseline_key = key
                self._sharding_mode = None
            self._key_same = None if (off_device or sd is None) else (sd, self.adj, self.features, self.features.data_ptr(), want2w)
        refreshed = created and not lt_dist.collectives_on()      # a new baseline computes everything on first use
        if getattr(self, "_sharding_mode", None) != mode:
            lt_dist.choose_baseline_sharding(self._baseline, mode=mode)      # (several ranks: ends with a refresh for `mode`)
            self._sharding_mode = mode
            refreshed = refreshed or lt_dist.collectives_on()
        if not refreshed:
            self._baseline.refresh(mode)
        return self._baseline

    def get_gradient_eps_mat(self, v):
        """attacker.py:100-108: (model(X + pert_v, A) - model(X, A)) / influence as an [N, C] tensor.
        Kept for API parity (one probe, all nodes observed); the attack itself uses the batched
        primitive and never materialises this matrix."""
        base = self.baseline("full")
        delta = float(self.args.influence)
        x = self.features
        xp = x.clone()
        xp[v] = x[v] + x[v] * delta
        w1, b1, w2, b2 = (p.to(x.device) for p in self._params())
        out_p = engine.gcn2_forward(base.graph, xp, w1, b1, w2, b2)
        return (out_p - base.logits()) / delta

    def get_gradient_eps(self, u, v):
        """attacker.py:89-97: row u of ``get_gradient_eps_mat(v)`` (API parity; the naive attack scores its pairs through
        ``pair_scores``)."""
        return self.get_gradient_eps_mat(v)[u]

    def _pair_route(self, mode=None):
        """The object whose ``influence_pairs`` scores a LIST of pairs for this model and mode, or None where the list has no
        primitive and the caller takes the rectangle (``_rows``).  The one place that decides it:
          * a 2-layer model served by ``engine.Baseline`` (lt_influence_pairs), every mode;
          * a 2-layer model with 9 .. 256 classes in ``delta`` (``engine.Baseline2W``, lt_influence2w_pairs: what ``baseline()``
            builds for it unless LT_WIDE2=slices);
          * a GCN3 with up to 8 classes (``engine.Baseline3``, lt_influence3_pairs), every mode;
          * a GCN3 with 9 .. 256 classes in ``delta`` (the wide handle; `sparse` / `full` keep the generic loop, as in ``_rows``).
        None for ``engine.WideBaseline``, generic stacks and CPU features.  The baseline is built or refreshed on the way, as in
        ``_rows``."""
        if not self.features.is_cuda:
            return None
        kind, sd = self._walk()
        m = self._mode(mode)
        if kind == "gcn2":
            base = self.baseline(m, sd)
            return base if isinstance(base, (engine.Baseline, engine.Baseline2W)) else None
        if kind == "gcn3" or (kind == "gcn3w" and m == "delta"):
            return self.baseline3(sd)
        return None

    def pair_scores(self, probe, observed, mode=None, chunk=1024) -> np.ndarray:
        """||grad_mat(probe[k])[observed[k]]||_2 for a LIST of pairs, float64 [n_pairs] on the host in input order.  A model
        with a pair-list primitive (``_pair_route``: a 2-layer model served by ``engine.Baseline`` or ``engine.Baseline2W``, a GCN3 within what
        ``engine.Baseline3`` serves) goes through ``influence_pairs``: the pairs grouped by probe (``engine.group_pairs``), one
        call, ONE device-to-host copy of n_pairs floats.  Every other model the attacker accepts (``engine.WideBaseline``,
        generic stacks, a GCN3 with more than 8 classes outside `delta`) takes ``_pair_scores_rect``: ``_rows`` on ``chunk``
        probes x the distinct observed nodes of their pairs, gathered -- the same values, through a rectangle."""
        probe = np.asarray(probe, dtype=np.int64).reshape(-1)
        observed = np.asarray(observed, dtype=np.int64).reshape(-1)
        if probe.shape != observed.shape:
            raise ValueError(f"probe and observed differ in length: {probe.size} / {observed.size}")
        n = int(self.features.shape[0])
        for ids, what in ((probe, "probe"), (observed, "observed")):      # (features[v] / grad[u] raise it in the reference)
            if ids.size and (int(ids.min()) < 0 or int(ids.max()) >= n):
                raise IndexError(f"{what}: node id out of range for {n} nodes")
        scores = np.empty(probe.size, dtype=np.float64)
        if probe.size == 0:
            return scores
        nodes, ptr, obs, order = engine.group_pairs(probe, observed)
        base = self._pair_route(mode)
        if base is not None:
            out = base.influence_pairs(nodes, ptr, obs, float(self.args.influence), self._mode(mode))
            scores[order] = out.cpu().numpy()
            engine.node_check()
            return scores
        return self._pair_scores_rect(nodes, ptr, obs, order, scores, mode, chunk)

    def _pair_scores_rect(self, nodes, ptr, obs, order, scores, mode=None, chunk=1024) -> np.ndarray:
        """The rectangle route of ``pair_scores`` (``engine.group_pairs``' layout in, ``scores`` filled in input order): the
        fallback of the models without a pair-list primitive, and what the list route is measured against."""
        for c0 in range(0, len(nodes), chunk):
            pc = nodes[c0:c0 + chunk]
            k0, k1 = int(ptr[c0]), int(ptr[c0 + len(pc)])
            cols, inv = np.unique(obs[k0:k1], return_inverse=True)
            rows = self._rows(pc.astype(np.int64), cols.astype(np.int64), mode).cpu().numpy().astype(np.float64)
            ridx = np.repeat(np.arange(len(pc)), np.diff(ptr[c0:c0 + len(pc) + 1]))
            scores[order[k0:k1]] = rows[ridx, inv.reshape(-1)]
        return scores

    def naive_result_filename(self):
        """attacker.py:181-184: the naive attack's file carries no attack-mode prefix."""
        a = self.args
        folder = f"eval_{self.dataset}"
        if a.mode == "vanilla-clean":
            return osp.join(folder, f"{a.sample_type}_{a.n_test}_{a.sample_seed}.pt")
        return osp.join(folder, f"{a.sample_type}_{a.perturb_type}_{a.n_test}_{a.sample_seed}"
                                f"_eps-{a.epsilon}_seed-{a.noise_seed}.pt")

    def link_prediction_attack(self):
        """The naive attack (``--attack-mode naive``, attacker.py:143-201): every sampled (u, v) is scored by perturbing v and
        reading ||grad[u]|| -- the existing pairs, then the non-existing ones, one ``pair_scores`` call each (the reference's
        two timed loops of two full forwards per pair), its prints and its result file."""
        t = time.time()
        ex = np.asarray(self.exist_edges, dtype=np.int64).reshape(-1, 2)
        norm_exist = list(self.pair_scores(ex[:, 1], ex[:, 0]))
        print(f"time for predicting existing edges: {time.time() - t}")
        t = time.time()
        nex = np.asarray(self.nonexist_edges, dtype=np.int64).reshape(-1, 2)
        norm_nonexist = list(self.pair_scores(nex[:, 1], nex[:, 0]))
        print(f"time for predicting non-existing edges: {time.time() - t}")
        self.compute_and_save(norm_exist, norm_nonexist, filename=self.naive_result_filename(), announce=False)

    def influence_matrix(self, mode=None) -> np.ndarray:
        """influence_val[i][j] = ||grad_mat(test_nodes[i])[test_nodes[j]]||_2 (attacker.py:216-229)
        as float64 [n_test, n_test] on the host.  Probes are sharded over ranks when
        torch.distributed is initialised (one all-gather of row slabs)."""
        nodes = np.asarray(self.test_nodes, dtype=np.int64)
        rank, ws = lt_dist.world()
        b, e, _ = lt_dist.shard_bounds(len(nodes), rank, ws)
        probes, observed = self._device_nodes(nodes, b, e)
        if ws == 1 and not lt_dist.collectives_on() and self.features.is_cuda:
            # one rank: the library call that forms the rows also lands them on the host as float64 (lt_influence_rows_f64)
            kind, sd = self._walk()
            if kind == "gcn2":
                m = self._mode(mode)
                base = self.baseline(m, sd)
                if isinstance(base, engine.Baseline):
                    return base.influence_matrix_host(probes, observed, float(self.args.influence), m)
        sharded = True
        if lt_dist.collectives_on():
            # several ranks: shard the probes + one all-gather, or -- when that measures slower than a rank doing every probe
            # itself (LT_SHARD_PROBES=auto: a build that is mostly its loop-invariant baseline) -- no collective at all
            all_p, _ = self._device_nodes(nodes, 0, len(nodes))
            key = ("attack", id(self.adj), self.features.data_ptr(), len(nodes), nodes[:8].tobytes(), self._mode(mode))
            sharded = lt_dist.choose_probe_sharding(
                key, lambda: lt_dist.all_gather_rows(self._rows(probes, observed, mode), len(nodes)),
                lambda: self._rows(all_p, observed, mode))
            if not sharded:
                probes = all_p
        local = None
        if sharded and lt_dist.collectives_on() and self._walk()[0] == "gcn2" and self._mode(mode) == "delta":
            # `delta` on the on-demand route (large graphs): the hub rows every rank's probes reach are formed once across the
            # ranks and exchanged (dist.SharedHubRows) instead of by every rank
            kind, sd = self._walk()
            base = self.baseline("delta", sd)
            if isinstance(base, engine.Baseline) and base.fp64_route() == 2:
                hkey = (id(base), nodes.tobytes())
                hub = getattr(self, "_hub_rows", None)
                if hub is None or hub[0] != hkey:
                    hub = self._hub_rows = (hkey, lt_dist.SharedHubRows(base, observed))
                hub[1].exchange()
                local = base.influence_rows(probes, observed, float(self.args.influence), "delta")
        if local is None:
            local = self._rows(probes, observed, mode)
        full = lt_dist.all_gather_rows(local, len(nodes)) if sharded else local
        if full.is_cuda:
            # ONE launch widens the rows on the device and writes them into pinned host memory; one wait (the reference:
            # n_test**2 `.item()` round trips into np.zeros -> float64, attacker.py:216-229)
            return engine.export_rows_f64(full)
        return full.numpy().astype(np.float64)

    def link_prediction_attack_efficient(self):
        t = time.time()
        self.influence_val = influence_val = self.influence_matrix()
        print(f"time for predicting edges: {time.time() - t}")

        node2ind = np.full(int(max(self.test_nodes)) + 1, -1, dtype=np.int64)
        node2ind[np.asarray(self.test_nodes, dtype=np.int64)] = np.arange(len(self.test_nodes))

        def scores(pairs):
            pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
            # perturb v, observe u: influence_val[ind[v]][ind[u]]   (attacker.py:236-245)
            # list of numpy float64 scalars, exactly what the reference appends (attacker.py:239,245)
            return list(influence_val[node2ind[pairs[:, 1]], node2ind[pairs[:, 0]]])

        self.compute_and_save(scores(self.exist_edges), scores(self.nonexist_edges))

    def link_prediction_attack_efficient_balanced(self, chunk=1024):
        """attacker.py:250-284 (``balanced-full``): for every node u that starts a pair, perturb u and
        read ||grad[v]|| for its partners v.  Scores are emitted grouped by u ascending -- edges of u,
        then non-edges of u, each in list order -- exactly as the reference appends them."""
        t = time.time()
        ex = np.asarray(self.exist_edges, dtype=np.int64).reshape(-1, 2)
        nex = np.asarray(self.nonexist_edges, dtype=np.int64).reshape(-1, 2)
        s_ex = np.empty(len(ex)); s_nex = np.empty(len(nex))
        if self._pair_route() is not None:
            # only the listed pairs are formed (lt_influence_pairs / lt_influence3_pairs: probe = the first node, observed = the
            # second), and only their scores cross PCIe -- the rows path forms chunk x N scores to read a few dozen per row; same bits
            s = self.pair_scores(np.concatenate([ex[:, 0], nex[:, 0]]), np.concatenate([ex[:, 1], nex[:, 1]]))
            s_ex[:], s_nex[:] = s[:len(ex)], s[len(ex):]
        else:
            self._balanced_scores_rect(ex, nex, s_ex, s_nex, chunk)
        print(f"time for predicting edges: {time.time() - t}")
        # stable sort by the first node reproduces the reference's grouped emission order
        oe, on = np.argsort(ex[:, 0], kind="stable"), np.argsort(nex[:, 0], kind="stable")
        self.compute_and_save(list(s_ex[oe]), list(s_nex[on]))

    def _balanced_scores_rect(self, ex, nex, s_ex, s_nex, chunk=1024):
        """The rectangle route of ``link_prediction_attack_efficient_balanced``: ``chunk`` starting nodes x every node through
        ``_rows``, each block copied to the host and read at the listed cells into ``s_ex`` / ``s_nex`` (list order).  The fallback
        of the models without a pair-list primitive, and what the list route is measured against."""
        n = self.worker.n_nodes
        starts = np.union1d(ex[:, 0], nex[:, 0])
        all_nodes = np.arange(n, dtype=np.int64)
        pos = np.full(n, -1, dtype=np.int64)
        for c0 in range(0, len(starts), chunk):
            probes = starts[c0:c0 + chunk]
            rows = self._rows(probes, all_nodes).cpu().numpy().astype(np.float64)
            pos[:] = -1
            pos[probes] = np.arange(len(probes))
            for pairs, dst in ((ex, s_ex), (nex, s_nex)):
                sel = pos[pairs[:, 0]] >= 0
                dst[sel] = rows[pos[pairs[sel, 0]], pairs[sel, 1]]
        return s_ex, s_nex

    # ------------------------------------------------------------------------------------------
    # recover_edges(chunk=K) / recover_graph: chunk e's rows formed against observed[:e] only (the cells right of the diagonal are
    # never read).  Off by default: every chunk then has an observed list of its own.  tools/recover_stream_time.py part (a) times
    # both forms; NOTES.md (2026-10-20) records what was measured and the decision
    recover_triangular = False

    # the baselines' streamed rows: chunk e's band formed over columns [0, e - 1) only (the square is symmetric, so the trapezoid is
    # half the products).  tools/corr_stream_time.py times both forms
    corr_trapezoid = True

    def _influence_row_source(self, probes, observed, mode=None):
        """The efficient attack's row source for ``_stream_top_pairs``: rows [b, e) of the influence matrix through ``_rows``."""
        def source(b, e, n_cols):
            obs = observed[:e] if (self.recover_triangular and e > 1) else observed
            return self._rows(probes[b:e], obs, mode)
        return source

    def _corr_row_source(self, observed, chunk):
        """The baseline attacks' row source for ``_stream_top_pairs`` over the listed nodes ``observed`` (int32, device) ->
        ``(source, handle)``.  A zero-norm row raises the one-shot route's ``ValueError`` here, before any row is formed."""
        vec = self._baseline_vectors_device()
        handle = engine.CorrRows(vec, observed, min(int(chunk), int(observed.numel())))
        handle.info.check(nan_ok=False)     # (a zero-norm row makes whole rows NaN: the selection's set would be unspecified)

        def source(b, e, n_cols):
            return handle.rows(b, e - b, n_cols if self.corr_trapezoid else None)
        return source, handle

    def _stream_top_pairs(self, source, n, m, chunk, device, extra_bytes=0):
        """``engine.top_pairs_lower`` of an n x n score matrix without forming it at once: ``source(b, e, n_cols)`` returns rows
        [b, e) -- of which columns [0, n_cols), n_cols = max(e - 1, 1), are read -- ``chunk`` rows at a time, consumed by an
        ``engine.TopPairsStream`` -> the same ``(idx, score, info)``.  Leaves the handle's counters in
        ``self.recover_stream_stats`` (device bytes, pushes; with ``self.recover_keep_stats`` set, the compaction counts too;
        ``rows_device_bytes``: ``extra_bytes``, what the row source's own handle holds)."""
        n, chunk = int(n), int(chunk)
        if chunk < 1:
            raise ValueError(f"chunk = {chunk}: at least 1")
        chunk = min(chunk, n)
        sel = engine.TopPairsStream(n, m, chunk, device=device)
        try:
            pushes = 0
            for b in range(0, n, chunk):
                e = min(b + chunk, n)
                sel.push(source(b, e, max(e - 1, 1)), b)
                pushes += 1
            out = sel.finish()
            self.recover_stream_stats = {"device_bytes": sel.device_bytes, "pushes": pushes, "chunk": chunk}
            if extra_bytes:
                self.recover_stream_stats["rows_device_bytes"] = int(extra_bytes)
            if getattr(self, "recover_keep_stats", False):      # (a copy of the handle's counters: one wait)
                self.recover_stream_stats.update(sel.stats())
        finally:
            sel.close()
        return out

    def _stream_scores(self, probes, observed, m, chunk, mode=None):
        """``_stream_top_pairs`` over the rows of the attack mode at hand: influence rows (efficient), or bands of the correlation
        square of the listed nodes (baseline / baseline-feat on a device route; the host route forms its square in one piece)."""
        n, dev = int(observed.numel()), observed.device
        if int(chunk) < 1:
            raise ValueError(f"chunk = {chunk}: at least 1")
        if str(getattr(self.args, "attack_mode", "efficient")) in ("baseline", "baseline-feat"):
            if self._baseline_route() != "device":
                raise NotImplementedError("chunked recovery of the baseline attacks needs baseline_scores = 'device' or 'stream': "
                                          "the host route forms its correlation square in one piece")
            source, handle = self._corr_row_source(observed, chunk)
            return self._stream_top_pairs(source, n, m, chunk, dev, handle.device_bytes)
        return self._stream_top_pairs(self._influence_row_source(probes, observed, mode), n, m, chunk, dev)

    def recover_graph(self, beliefs=None, mode=None, chunk=1024, nodes=None) -> dict:
        """``recover_edges`` for the attacked graph itself: the node set is every node (or ``nodes``), each is perturbed, every
        pair is ranked, and the m highest-scoring pairs under each density belief are the predicted edges.  Needs no
        ``prepare_test_data()`` and no pair lists: the rows are formed ``chunk`` probes at a time and consumed by an
        ``engine.TopPairsStream`` (O(m) device state, no n x n matrix, no label triangle); the edge count comes from
        ``sampling.upper_edge_count`` on the device (a given ``nodes`` list: counted on the HOST in the scipy pattern restricted to
        the list, one pass over the stored entries -- the whole graph is the case the device count serves), ``is_edge`` from
        ``engine.pairs_present`` for the selected pairs only.  Returns and stores the ``recovered`` dict of ``recover_edges``, key
        for key.  Serves every model kind ``_rows`` serves; with several ranks every rank forms everything itself.  With
        ``attack_mode`` baseline / baseline-feat on a device route the rows are bands of the correlation square of the listed
        nodes (``engine.CorrRows`` over ``_baseline_vectors_device()``, the mean over the listed nodes)."""
        from . import recover, sampling
        n_graph = int(self.features.shape[0])
        nodes = np.arange(n_graph, dtype=np.int64) if nodes is None else np.asarray(nodes, dtype=np.int64).reshape(-1)
        n = len(nodes)
        if n < 2:
            raise ValueError("recover_graph: fewer than two nodes")
        if not self.features.is_cuda:
            raise engine._lib.LinkTellerHipError("recover_graph: the features must live on the GPU; there is no CPU path")
        n_total = n * (n - 1) // 2
        probes, observed = self._device_nodes(nodes, 0, n)
        csr = self._pattern_csr()
        if n == n_graph and np.array_equal(nodes, np.arange(n_graph)):
            n_edges = sampling.upper_edge_count(csr)
        else:
            import scipy.sparse as sp
            adj = sp.csr_matrix(self.worker.adj_ori)
            pattern = sp.csr_matrix((np.ones(adj.indices.shape[0], dtype=np.int8), adj.indices, adj.indptr), shape=adj.shape)
            sub = sp.coo_matrix(pattern[nodes][:, nodes])        # positions of the node list: pair (i, j), i < j, as the samplers count
            sub.sum_duplicates()
            n_edges = int((sub.col > sub.row).sum())
        beliefs = recover.density_ladder(n_edges, n) if beliefs is None else [float(b) for b in beliefs]
        counts = recover.belief_counts(beliefs, n_total)
        m = int(counts.max())
        idx_d, val_d, info = self._stream_scores(probes, observed, m, chunk, mode)
        # cell (i, j), j < i: the pair (nodes[j], nodes[i]) scored by perturbing nodes[i]
        obs64 = observed.to(torch.int64)
        present_d = engine.pairs_present(csr, obs64[idx_d % n], obs64[idx_d // n])
        idx, val, raw = idx_d.cpu().numpy(), val_d.cpu().numpy(), info["raw"].cpu().numpy()
        engine.node_check()
        order = np.lexsort((idx, -val.astype(np.float64)))      # ascending cell index -> rank order
        idx, val = idx[order], val[order]
        ci, cj = idx // n, idx % n
        u, v = nodes[cj], nodes[ci]
        present = present_d.cpu().numpy()[order] != 0
        stats = recover.recovery_stats(present, n_edges, counts)
        self.recovered = {
            "pairs": np.stack([u, v], axis=1).astype(np.int64), "scores": val.astype(np.float64), "is_edge": present,
            "beliefs": list(beliefs), "counts": counts, "precision": stats["precision"], "recall": stats["recall"],
            "f1": stats["f1"], "tp": stats["tp"],
            "threshold": float(np.array([raw[0]], dtype=np.int64).astype(np.uint32).view(np.float32)[0]),
            "n_edges": n_edges, "n_total": n_total,
            "above": int(raw[1]), "tied_taken": int(raw[2]), "tied_total": int(raw[3]),
        }
        return self.recovered

    def recovered_all_filename(self):
        name = self.result_filename()
        return osp.join(osp.dirname(name), "recover_all_" + osp.basename(name))

    def recover_edges(self, beliefs=None, mode=None, chunk=None) -> dict:
        """The attack's edge list (the reference's post-processing script, attack_stats_all.py:44-116): under a belief k about the
        density of the sampled subgraph, the m = ceil(k n (n - 1) / 2) highest-scoring pairs of sampled nodes are predicted as
        edges.  ``beliefs=None``: the reference's ladder r/4 .. 4r around the subgraph's true density (``recover.density_ladder``).
        The n_test x n_test rows are formed on the device (``_rows``: every model kind it serves) and stay there: ONE
        ``engine.top_pairs_lower`` call selects the largest m of the beliefs from their strict lower triangle -- cell (i, j), j < i,
        is the pair (test_nodes[j], test_nodes[i]) scored by perturbing test_nodes[i], as ``link_prediction_attack_efficient``
        reads it -- and m indices and scores cross PCIe instead of the matrix.  The order (score descending, then cell index) is
        total, so a smaller belief's prediction is a prefix of the ranked list.  Needs ``prepare_test_data()`` with an
        ``unbalanced*`` sample type.  With several ranks every rank forms all rows itself: no collective of its own to mismatch.
        For ``attack_mode`` baseline / baseline-feat with ``args.baseline_scores == "device"`` the rows are the correlation square
        of ``engine.corr_square`` (symmetric) instead of influence rows; a sampled node whose centred vector is zero makes its
        row NaN and raises ``ValueError`` (a ranking over NaNs is undefined).  ``chunk=K`` forms the rows K at a time
        (``_stream_scores``: influence rows, or bands of the correlation square through ``engine.CorrRows``, whose cells are the
        square's bit for bit) and returns the same dict, array for array."""
        from . import recover
        st = str(self.args.sample_type)
        if not st.startswith("unbalanced"):
            raise NotImplementedError(f"recover_edges: sample_type = {st} has no all-pairs square of sampled nodes "
                                      f"(unbalanced, unbalanced-lo, unbalanced-hi do)")
        nodes = np.asarray(self.test_nodes, dtype=np.int64)
        n = len(nodes)
        if n < 2:
            raise ValueError("recover_edges: fewer than two sampled nodes")
        n_total = n * (n - 1) // 2
        dev_sample = getattr(self, "_sample_dev", None)
        dev_sample = dev_sample if (dev_sample is not None and dev_sample["kind"] == "square" and self.features.is_cuda) else None
        probes, observed = self._device_nodes(nodes, 0, n)
        if dev_sample is not None:
            # the sample was prepared on the device: its edge count is info[0] of the label build (the wait of this call's set-up)
            _, tri, tri_info = self._square_lists(n, self.features.device)
            n_edges = self._square_n_edges(tri_info)
        else:
            n_edges = len(self.exist_edges)
        beliefs = recover.density_ladder(n_edges, n) if beliefs is None else [float(b) for b in beliefs]
        counts = recover.belief_counts(beliefs, n_total)
        m = int(counts.max())
        cinfo = None
        if chunk is not None:
            # addition: the rows chunk by chunk through engine.TopPairsStream -- the same triple, no n x n matrix
            # (the baseline attacks on a device route: bands of their correlation square, engine.CorrRows)
            idx_d, val_d, info = self._stream_scores(probes, observed, m, chunk, mode)
        elif str(getattr(self.args, "attack_mode", "efficient")) in ("baseline", "baseline-feat") and self._baseline_route() == "device":
            rows, cinfo = self._baseline_square_device()     # (addition: the baseline attacks' correlation square, symmetric)
            idx_d, val_d, info = engine.top_pairs_lower(rows, m)
        else:
            rows = self._rows(probes, observed, mode)
            idx_d, val_d, info = engine.top_pairs_lower(rows, m)
        if cinfo is not None:
            cinfo.check(nan_ok=False)     # (a zero-norm row makes whole rows NaN: lt_top_pairs_lower's set would be unspecified)
        if dev_sample is not None:
            # cell (i, j), j < i, is the pair of positions (j, i): slot j (2 n - j - 1) / 2 + (i - j - 1) of the label triangle
            ci_d, cj_d = idx_d // n, idx_d % n
            present_d = tri[cj_d * (2 * n - cj_d - 1) // 2 + (ci_d - cj_d - 1)]
        idx, val, raw = idx_d.cpu().numpy(), val_d.cpu().numpy(), info["raw"].cpu().numpy()
        engine.node_check()
        order = np.lexsort((idx, -val.astype(np.float64)))      # ascending cell index -> rank order
        idx, val = idx[order], val[order]
        ci, cj = idx // n, idx % n
        u, v = nodes[cj], nodes[ci]
        if dev_sample is not None:
            present = present_d.cpu().numpy()[order] != 0
        else:
            import scipy.sparse as sp
            adj = sp.csr_matrix(self.worker.adj_ori)
            pattern = sp.csr_matrix((np.ones(adj.indices.shape[0], dtype=np.int8), adj.indices, adj.indptr), shape=adj.shape)
            present = np.asarray(pattern[u, v]).reshape(-1) != 0     # structural presence of v in row u, as edge_sets_among_nodes reads it
        stats = recover.recovery_stats(present, n_edges, counts)
        self.recovered = {
            "pairs": np.stack([u, v], axis=1).astype(np.int64), "scores": val.astype(np.float64), "is_edge": present,
            "beliefs": list(beliefs), "counts": counts, "precision": stats["precision"], "recall": stats["recall"],
            "f1": stats["f1"], "tp": stats["tp"],
            "threshold": float(np.array([raw[0]], dtype=np.int64).astype(np.uint32).view(np.float32)[0]),
            "n_edges": n_edges, "n_total": n_total,
            "above": int(raw[1]), "tied_taken": int(raw[2]), "tied_total": int(raw[3]),
        }
        return self.recovered

    def recovered_filename(self):
        name = self.result_filename()
        return osp.join(osp.dirname(name), "recover_" + osp.basename(name))

    def save_recovered(self, filename=None):
        """The dict of ``recover_edges`` next to the attack's result file (``eval_<dataset>/recover_<result file>``), one printed
        line per belief.  Rank 0 only.  ``filename``: another place (``recovered_all_filename()`` for ``recover_graph``)."""
        rank, _ = lt_dist.world()
        if rank != 0:
            return
        r = self.recovered
        for k, b in enumerate(r["beliefs"]):
            print(f"belief = {b:.6g}, m = {int(r['counts'][k])}, tp = {int(r['tp'][k])}, precision = {r['precision'][k]:.4f}, "
                  f"recall = {r['recall'][k]:.4f}, f1 = {r['f1'][k]:.4f}")
        filename = self.recovered_filename() if filename is None else filename
        os.makedirs(osp.dirname(filename), exist_ok=True)
        torch.save(r, filename)
        print(f"recovered edges saved to: {filename}")

    # ------------------------------------------------------------------------------------------
    def _metric_lists(self, lds, dev):
        """(index, labels) of the efficient attack's sampled pairs on the device: pair (u, v) -- perturb v, observe u -- is the
        storage element ``ind[v] * lds + ind[u]`` of the rows, the cell ``link_prediction_attack_efficient`` reads; the existing
        pairs first (label 1), then the others.  Built once per sample on the host and uploaded once: the cache holds the very
        edge lists it was built from, so a new ``prepare_test_data()`` (new list objects) replaces it."""
        c = getattr(self, "_metric_cache", None)
        if (c is not None and c[0] is self.exist_edges and c[1] is self.nonexist_edges and c[2] is self.test_nodes
                and c[3] == (lds, dev)):
            return c[4], c[5]
        nodes = np.asarray(self.test_nodes, dtype=np.int64)
        node2ind = np.full(int(nodes.max()) + 1, -1, dtype=np.int64)
        node2ind[nodes] = np.arange(len(nodes))
        ex = np.asarray(self.exist_edges, dtype=np.int64).reshape(-1, 2)
        nex = np.asarray(self.nonexist_edges, dtype=np.int64).reshape(-1, 2)
        pairs = np.concatenate([ex, nex])
        if pairs.size and (pairs.min() < 0 or pairs.max() >= node2ind.size or (node2ind[pairs] < 0).any()):
            raise IndexError("a sampled pair names a node outside the sampled nodes")
        index = node2ind[pairs[:, 1]] * int(lds) + node2ind[pairs[:, 0]]
        labels = np.zeros(len(pairs), dtype=np.uint8)
        labels[:len(ex)] = 1
        index_t, labels_t = torch.from_numpy(index).to(dev), torch.from_numpy(labels).to(dev)
        self._metric_cache = (self.exist_edges, self.nonexist_edges, self.test_nodes, (lds, dev), index_t, labels_t)
        return index_t, labels_t

    def _pair_curve(self, probe, observed, labels, mode=None):
        """``engine.score_curve`` over a LIST of pairs: straight from the device tensor ``Baseline.influence_pairs`` returns where
        ``pair_scores`` takes that route (the labels permuted as ``engine.group_pairs`` orders the pairs), else from
        ``pair_scores``' host result, uploaded (fp32 values widened on the way down: the narrowing is exact)."""
        dev = self.features.device
        base = self._pair_route(mode)
        if base is not None:
            n = int(self.features.shape[0])
            for ids, what in ((probe, "probe"), (observed, "observed")):
                if ids.size and (int(ids.min()) < 0 or int(ids.max()) >= n):
                    raise IndexError(f"{what}: node id out of range for {n} nodes")
            nodes, ptr, obs, order = engine.group_pairs(probe, observed)
            out = base.influence_pairs(nodes, ptr, obs, float(self.args.influence), self._mode(mode))
            return engine.score_curve(out, torch.from_numpy(np.ascontiguousarray(labels[order])).to(dev))
        s = self.pair_scores(probe, observed, mode)
        if not self.features.is_cuda:
            raise LinkTellerHipError("evaluate: the metrics run on the GPU; there is no CPU path")
        return engine.score_curve(torch.from_numpy(s.astype(np.float32)).to(dev), torch.from_numpy(labels).to(dev))

    def _pair_curve_device(self, probe, observed, n_edges, mode=None):
        """``_pair_curve`` for pair lists that live on the device (int32 CUDA tensors, the first ``n_edges`` pairs labelled 1):
        ``engine.group_pairs_device`` + ``Baseline.influence_pairs`` + ``engine.score_curve``, the labels permuted by the device
        ``order``.  None when the model has no pair-list primitive (``_pair_route``; the caller takes the host lists)."""
        if not self.features.is_cuda or probe.numel() == 0:
            return None
        base = self._pair_route(mode)
        if base is None:
            return None
        nodes, ptr, obs, order = engine.group_pairs_device(probe, observed, int(self.features.shape[0]))
        out = base.influence_pairs(nodes, ptr, obs, float(self.args.influence), self._mode(mode))
        labels = torch.zeros(probe.numel(), dtype=torch.uint8, device=probe.device)
        labels[:n_edges] = 1
        return engine.score_curve(out, labels[order.long()])

    def evaluate(self, mode=None, curves=False) -> dict:
        """AUC and AP of the attack without the host's three sorts (the reference's ``compute_and_save``, attacker.py:378-389,
        minus its file): the scores stay on the device, ``engine.score_curve`` ranks and counts them there, and eight words --
        with ``curves=True`` also the D distinct thresholds' counts -- cross PCIe.  Sets ``self.auc`` (the exact Mann-Whitney
        value ``auc2 / (2 P N)``; the trapezoid of ``compute_and_save`` agrees to rounding) and ``self.ap``, prints the same two
        lines, writes no file.  Returns ``{"auc", "ap", "n_thresholds", "n_pos", "n_neg"}``, with ``curves=True`` also
        ``"curves"``: ``metrics.curves_from_counts(...)``, the arrays ``compute_and_save`` stores, bit for bit.  Needs
        ``prepare_test_data()``.  Efficient attack on an ``unbalanced*`` sample: the n_test x n_test rows of ``_rows`` (every
        model kind it serves) read through a cached index; naive attack and ``balanced-full``: the listed pairs' scores.  The
        baseline attacks' scores are host arithmetic: ``NotImplementedError`` -- unless ``args.baseline_scores == "device"``: then
        their square (``engine.corr_square``) is read through the same index, their pair list is ``engine.corr_pairs``'.  After ``prepare_test_data(pairs="device")`` the
        square's labels and index are ``sampling.square_labels_device``'s, after ``prepare_test_data(rng="philox")`` the pair
        lists are grouped on the device (``_pair_curve_device``); no host pair list is built for either.  With several ranks every rank forms all rows
        itself: no collective of its own to mismatch."""
        from . import metrics as lt_metrics
        am = str(getattr(self.args, "attack_mode", "efficient"))
        st = str(self.args.sample_type)
        corr_info = None
        if am in ("baseline", "baseline-feat") and self._baseline_route() != "device":
            raise NotImplementedError(f"evaluate: attack_mode = {am} scores its pairs on the host (baseline_attack)")
        if am not in ("efficient", "naive", "baseline", "baseline-feat"):
            raise NotImplementedError(f"attack_mode = {am} not implemented!")
        dev_sample = getattr(self, "_sample_dev", None) if self.features.is_cuda else None
        curve = tri_info = None
        if am in ("baseline", "baseline-feat"):
            # baseline_scores = device: the correlations are formed on the device and stay there (corr_square / corr_pairs)
            if st.startswith("unbalanced"):
                nodes = np.asarray(self.test_nodes, dtype=np.int64)
                rows, corr_info = self._baseline_square_device()
                lds = int(rows.shape[1])
                # the square is symmetric bit for bit: the efficient attack's cell (ind[v], ind[u]) holds the pair's score
                if dev_sample is not None and dev_sample["kind"] == "square" and len(nodes) > 1:
                    index, labels, tri_info = self._square_lists(lds, rows.device)
                else:
                    index, labels = self._metric_lists(lds, rows.device)
                curve = engine.score_curve(rows, labels, index)
            elif st == "balanced-full":
                vec = self._baseline_vectors_device()
                if dev_sample is not None and dev_sample["kind"] == "balanced":      # the philox pair lists never left the device
                    u, v, n_edges = dev_sample["u"], dev_sample["v"], int(dev_sample["n_edges"])
                    labels = torch.zeros(u.numel(), dtype=torch.uint8, device=u.device)
                    labels[:n_edges] = 1
                else:
                    u, v, labels = self._baseline_pair_lists(vec.device)
                scores, corr_info = engine.corr_pairs(vec, u, v)
                curve = engine.score_curve(scores, labels)
            else:
                raise NotImplementedError(f"sample_type = {st} not implemented!")
            corr_info.check()                                    # (IndexError before the NaN cells of a bad id reach the curve)
        elif am == "efficient" and st.startswith("unbalanced"):
            nodes = np.asarray(self.test_nodes, dtype=np.int64)
            probes, observed = self._device_nodes(nodes, 0, len(nodes))
            rows = self._rows(probes, observed, mode)
            lds = int(rows.stride(0)) if rows.shape[0] > 1 else int(rows.shape[1])
            if dev_sample is not None and dev_sample["kind"] == "square" and len(nodes) > 1:
                index, labels, tri_info = self._square_lists(lds, rows.device)     # (prepared on the device: no host pair list)
            else:
                index, labels = self._metric_lists(lds, rows.device)
            curve = engine.score_curve(rows, labels, index)
        elif dev_sample is not None and dev_sample["kind"] == "balanced":
            # the philox pair lists never left the device: perturb u, observe v (efficient) / perturb v, observe u (naive)
            p, o = (dev_sample["v"], dev_sample["u"]) if am == "naive" else (dev_sample["u"], dev_sample["v"])
            curve = self._pair_curve_device(p, o, dev_sample["n_edges"], mode)
        if curve is None:
            ex = np.asarray(self.exist_edges, dtype=np.int64).reshape(-1, 2)
            nex = np.asarray(self.nonexist_edges, dtype=np.int64).reshape(-1, 2)
            labels = np.zeros(len(ex) + len(nex), dtype=np.uint8)
            labels[:len(ex)] = 1
            # naive (attacker.py:143-163): perturb v, observe u; balanced-full (attacker.py:250-284): perturb u, observe v
            p, o = (1, 0) if am == "naive" else (0, 1)
            curve = self._pair_curve(np.concatenate([ex[:, p], nex[:, p]]), np.concatenate([ex[:, o], nex[:, o]]), labels, mode)
        out = curve.summary()                                    # the wait
        engine.node_check()
        if tri_info is not None:
            self._square_n_edges(tri_info)                       # (the device's check of the sampled nodes, once per sample)
        self.auc, self.ap = out["auc"], out["ap"]
        print("auc =", self.auc)
        print("ap =", self.ap)
        if curves:
            out["curves"] = lt_metrics.curves_from_counts(*curve.counts())
        return out

    # ------------------------------------------------------------------------------------------
    def _baseline_vectors(self):
        """attacker.py:295-303: softmax posteriors (sigmoid for ppi) or the raw features, float32 on host."""
        am = self.args.attack_mode
        if am == "baseline":
            with torch.no_grad():
                out = self.model(self.features, self.adj)
                post = torch.softmax(out, dim=1) if self.dataset != "ppi" else torch.sigmoid(out)
            return post.float().cpu()
        if am == "baseline-feat":
            return self.features.float().cpu()
        raise NotImplementedError(f"attack_mode={am} not implemented!")

    # ---- baseline_scores = device (an addition) -----------------------------------------------------------
    def _baseline_route(self):
        route = getattr(self.args, "baseline_scores", "host")
        if route != "host" and route not in DEVICE_BASELINE_SCORES:
            raise ValueError(f"baseline_scores = {route!r}: 'host', 'device' or 'stream'")
        # 'stream' is the device route; it differs on the command line only, where it also admits the chunked recovery
        return "device" if route in DEVICE_BASELINE_SCORES else route

    def _baseline_vectors_device(self):
        """The vectors of ``_baseline_vectors``, left on the device: softmax (sigmoid for ppi) of the model's output, or the
        features.  The softmax / sigmoid is a torch op on the device tensor."""
        if not self.features.is_cuda:
            raise LinkTellerHipError("baseline_scores = device: the scores are formed on the GPU; there is no CPU path")
        am = self.args.attack_mode
        if am == "baseline":
            with torch.no_grad():
                out = self.model(self.features, self.adj)
                post = torch.softmax(out, dim=1) if self.dataset != "ppi" else torch.sigmoid(out)
            return post.float()
        if am == "baseline-feat":
            return self.features.float()
        raise NotImplementedError(f"attack_mode={am} not implemented!")

    def _baseline_square_device(self):
        """(square, info) of ``engine.corr_square`` over the sampled nodes: fp32 [n_test, n_test] on the device."""
        vec = self._baseline_vectors_device()
        nodes = np.asarray(self.test_nodes, dtype=np.int64)
        _, observed = self._device_nodes(nodes, 0, len(nodes))
        return engine.corr_square(vec, observed)

    def _baseline_pair_lists(self, dev):
        """(u, v, labels) of the host pair lists on the device: the existing pairs first (label 1), then the others."""
        ex = np.asarray(self.exist_edges, dtype=np.int64).reshape(-1, 2)
        nex = np.asarray(self.nonexist_edges, dtype=np.int64).reshape(-1, 2)
        pairs = np.concatenate([ex, nex])
        n = int(self.features.shape[0])
        if pairs.size and (pairs.min() < 0 or pairs.max() >= n):
            raise IndexError(f"a sampled pair names a node outside the {n} nodes")
        labels = np.zeros(len(pairs), dtype=np.uint8)
        labels[:len(ex)] = 1
        u = torch.from_numpy(np.ascontiguousarray(pairs[:, 0], dtype=np.int32)).to(dev)
        v = torch.from_numpy(np.ascontiguousarray(pairs[:, 1], dtype=np.int32)).to(dev)
        return u, v, torch.from_numpy(labels).to(dev)

    def baseline_attack(self):
        """LSA2-post / LSA2-attr, attacker.py:287-334: correlation of mean-centred vectors, the mean taken
        over the sampled nodes; fp32 arithmetic, scores widened to float64 like the reference's matrix.
        ``args.baseline_scores == "device"``: the square is ``engine.corr_square``'s (fp64 arithmetic, one rounding to fp32), one
        copy brings it back; the same pairs are read from it and the same file is written."""
        t = time.time()
        nodes = torch.as_tensor(np.asarray(self.test_nodes, dtype=np.int64))
        if self._baseline_route() == "device":
            sq, cinfo = self._baseline_square_device()
            corr = sq.cpu().numpy().astype(np.float64)
            cinfo.check()
        else:
            vec = self._baseline_vectors()
            d = vec[nodes] - torch.mean(vec[nodes], dim=0)
            nrm = torch.norm(d, dim=1)
            corr = ((d @ d.T) / nrm[:, None] / nrm[None, :]).numpy().astype(np.float64)
        print(f"time for computing correlation value: {time.time() - t}")
        node2ind = np.full(int(nodes.max()) + 1, -1, dtype=np.int64)
        node2ind[nodes.numpy()] = np.arange(len(nodes))

        def scores(pairs):
            pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
            i, j = node2ind[pairs[:, 0]], node2ind[pairs[:, 1]]
            return list(corr[np.minimum(i, j), np.maximum(i, j)])

        self.compute_and_save(scores(self.exist_edges), scores(self.nonexist_edges))

    def baseline_attack_balanced(self):
        """attacker.py:337-375: same correlation with the mean over all nodes, one value per listed pair.
        ``args.baseline_scores == "device"``: the scores are ``engine.corr_pairs``', one copy of one float per pair."""
        t = time.time()
        if self._baseline_route() == "device":
            vec = self._baseline_vectors_device()
            u, v, labels = self._baseline_pair_lists(vec.device)
            out, cinfo = engine.corr_pairs(vec, u, v)
            s = out.cpu().numpy().astype(np.float64)
            cinfo.check()
            n_ex = len(np.asarray(self.exist_edges, dtype=np.int64).reshape(-1, 2))
            print(f"time for computing correlation value: {time.time() - t}")
            self.compute_and_save(list(s[:n_ex]), list(s[n_ex:]))
            return
        vec = self._baseline_vectors()
        d = vec - torch.mean(vec, dim=0)
        nrm = torch.norm(d, dim=1)

        def scores(pairs):
            pairs = torch.as_tensor(np.asarray(pairs, dtype=np.int64).reshape(-1, 2))
            u, v = pairs[:, 0], pairs[:, 1]
            return list(((d[u] * d[v]).sum(dim=1) / nrm[u] / nrm[v]).numpy().astype(np.float64))

        se, sn = scores(self.exist_edges), scores(self.nonexist_edges)
        print(f"time for computing correlation value: {time.time() - t}")
        self.compute_and_save(se, sn)

    # ------------------------------------------------------------------------------------------
    def result_filename(self):
        a = self.args
        folder = f"eval_{self.dataset}"
        if a.mode == "vanilla-clean":                        # attacker.py:391-394
            name = f"{a.attack_mode}_{a.sample_type}_{a.n_test}_{a.sample_seed}.pt"
        else:
            name = (f"{a.attack_mode}_{a.sample_type}_{a.perturb_type}_{a.n_test}_{a.sample_seed}"
                    f"_eps-{a.epsilon}_seed-{a.noise_seed}.pt")
        return osp.join(folder, name)

    def compute_and_save(self, norm_exist, norm_nonexist, filename=None, announce=True):
        """attacker.py:378-412: sklearn ROC / PR on the host, same prints, same ``.pt`` schema.  ``filename`` / ``announce``:
        the naive attack writes the same dict under its own name and prints no "saved" line (attacker.py:165-201)."""
        y = [1] * len(norm_exist) + [0] * len(norm_nonexist)
        pred = list(norm_exist) + list(norm_nonexist)

        fpr, tpr, thresholds = metrics.roc_curve(y, pred)
        self.auc = metrics.auc(fpr, tpr)
        print("auc =", self.auc)
        precision, recall, thresholds_2 = metrics.precision_recall_curve(y, pred)
        self.ap = metrics.average_precision_score(y, pred)
        print("ap =", self.ap)

        rank, _ = lt_dist.world()
        if rank != 0:
            return
        filename = filename or self.result_filename()
        os.makedirs(osp.dirname(filename), exist_ok=True)
        torch.save({
            "auc": {"fpr": fpr, "tpr": tpr, "thresholds": thresholds},
            "pr": {"precision": precision, "recall": recall, "thresholds": thresholds_2},
            "result": {"y": y, "pred": pred},
        }, filename)
        if announce:
            print(f"attack results saved to: {filename}")
