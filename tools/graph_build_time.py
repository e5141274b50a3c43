"""Wall time of a fresh graph create, host builder against device builder, in one process on one GPU.

Graphs: the twitch-RU-shaped Erdos-Renyi graph of bench.py (N = 4385, incidence records built), the power-law graph of the same
size (hub rows: no records), and with --rmat the R-MAT scale-21 graph of BASELINE configs[4].  Per graph, `--reps` (>= 10) fresh
creates per builder, the four builders taking turns inside every repetition:

  host_csr      lt_graph_create from a host CSR (validation, every table on the host, the uploads)
  device_csr    lt_graph_create_device from a device-resident CSR, synchronised
  api_host      as_hip_graph(cuda sparse tensor) under LT_GRAPH_BUILD=host (tensor -> CPU -> scipy -> host builder: what a CLI
                run paid before the device builder)
  api_auto      the same call under LT_GRAPH_BUILD=auto (coalesce on the device, row pointers by torch, device builder)

Every create is followed by a device synchronisation inside the timed region and the graph is destroyed outside it.  Reports
median, min and max in milliseconds and writes profiles/graph_build_time.json (`python tools/graph_build_time.py [--rmat]`)."""
import argparse
import ctypes as C
import gc
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=15)
    p.add_argument("--rmat", action="store_true", help="also the R-MAT scale-21 graph (a minute of host time to generate)")
    p.add_argument("--rmat-scale", type=int, default=21)
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "graph_build_time.json"))
    a = p.parse_args()
    a.reps = max(a.reps, 10)

    import torch
    from linkteller_amd import _lib, graph, synth
    dev = torch.device("cuda:0")
    h = _lib.lib()
    shp = synth.TWITCH_SHAPES["twitch-RU"]
    graphs = [("twitch-RU ER", graph.first_order_gcn(synth.erdos_renyi_graph(shp["n"], shp["e"], seed=0))),
              ("twitch-RU power-law", graph.first_order_gcn(synth.powerlaw_graph(shp["n"], shp["e"], seed=0)))]
    if a.rmat:
        graphs.append((f"R-MAT scale {a.rmat_scale}",
                       graph.first_order_gcn(synth.rmat_graph(a.rmat_scale, synth.rmat_draws(a.rmat_scale), seed=42))))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g = fn()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        return dt, g

    results = []
    for name, mat in graphs:
        n, rowptr, col, val = graph.csr_arrays(mat)
        nnz = len(col)
        d_rowptr, d_col, d_val = (torch.from_numpy(x).to(dev) for x in (rowptr, col, val))
        coo = mat.tocoo()
        idx = torch.from_numpy(np.vstack((coo.row, coo.col)).astype(np.int64)).to(dev)
        vals = torch.from_numpy(coo.data.astype(np.float32)).to(dev)

        def host_csr():
            out = C.c_void_p()
            _lib.check(h.lt_graph_create(n, nnz, rowptr.ctypes.data, col.ctypes.data, val.ctypes.data, C.byref(out)), "lt_graph_create")
            return out

        def device_csr():
            out = C.c_void_p()
            _lib.check(h.lt_graph_create_device(n, nnz, d_rowptr.data_ptr(), d_col.data_ptr(), d_val.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream, C.byref(out)), "lt_graph_create_device")
            return out

        def api(mode):
            def run():
                os.environ["LT_GRAPH_BUILD"] = mode
                # (a fresh tensor object per call: as_hip_graph caches per object)
                return graph.as_hip_graph(torch.sparse_coo_tensor(idx, vals, mat.shape))
            return run

        builders = [("host_csr", host_csr), ("device_csr", device_csr), ("api_host", api("host")), ("api_auto", api("auto"))]
        times = {k: [] for k, _ in builders}
        built_on = {}
        records = None
        for rep in range(a.reps + 2):                          # two warm-up repetitions (first kernel loads, allocator pools)
            for k, fn in builders:
                dt, g = timed(fn)
                if isinstance(g, graph.HipGraph):
                    built_on[k] = g.built_on
                    if records is None:
                        records = bool(g.scalars()["has_records"])
                    del g
                    gc.collect()
                else:
                    h.lt_graph_destroy(g)
                if rep >= 2:
                    times[k].append(dt)
        os.environ.pop("LT_GRAPH_BUILD", None)
        assert built_on == {"api_host": "host", "api_auto": "device"}, built_on
        row = {"graph": name, "n": n, "nnz": nnz, "records": records, "reps": a.reps,
               "ms": {k: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for k, v in times.items()}}
        results.append(row)
        print(f"{name}: n={n} nnz={nnz} records={records}")
        for k, v in row["ms"].items():
            print(f"  {k:11s} median {v['median']:9.3f} ms   min {v['min']:9.3f}   max {v['max']:9.3f}")
        hm, dm = row["ms"]["host_csr"], row["ms"]["device_csr"]
        print(f"  host median - device median = {hm['median'] - dm['median']:.3f} ms; host spread (max - min) = {hm['max'] - hm['min']:.3f} ms")
        os.makedirs(os.path.dirname(a.out), exist_ok=True)          # (after every graph: the R-MAT leg takes minutes)
        with open(a.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "host_cpus": len(os.sched_getaffinity(0)), "results": results}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
