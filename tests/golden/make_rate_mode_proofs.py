#!/usr/bin/env python3
"""Writes tests/golden/rate_mode_proofs.json: one mode-3 and one mode-4 'ZKSR' proof (stark.prove_rate_modes) at blow-up 4 with 1 query and 0 grinding bits — the runs
`timestamps` (8 rows: two stores and two loads on one cell) and `sha256_hello` (21 rows: one SHA-256 call, the hash tape, the boundary cell) of tests/programs.py, moved
off the code segment as the GPU tests take them.  tests/test_prove_rate_modes_verify.py checks zkir_verify_rate on them without a GPU.

What this pins: the PRODUCT's own output, frozen — the oracle has no prover for these modes at another rate, so nothing here is held against an outside reference (the
GPU tests hold the parts of such a proof against the oracle: tests/test_gpu_prove_rate_modes.py).  Regenerate only when the format changes on purpose.

Needs the GPU (the proofs come from the GPU prover): python tests/golden/make_rate_mode_proofs.py [output path]
The words are stored as base64 of the zlib-compressed little-endian u32 words; `sha256` is of the uncompressed bytes.
"""
import base64
import hashlib
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

CASES = {"mode3": ("timestamps", False), "mode4": ("sha256_hello", True)}
LOG_BLOWUP, NUM_QUERIES, POW_BITS = 2, 1, 0


def main(out_path):
    import programs as pg
    from zkir_amd import pipeline as pl, runtime as rt, stark
    doc = {"_about": "mode-3 and mode-4 'ZKSR' proofs from the GPU prover (tests/golden/make_rate_mode_proofs.py): the product's own output, frozen; pins nothing "
                     "against an outside reference.  words: base64(zlib(little-endian u32 words)).",
           "log_blowup": LOG_BLOWUP, "num_queries": NUM_QUERIES, "pow_bits": POW_BITS, "proofs": {}}
    for key, (which, wide) in CASES.items():
        blob, ins, cfg = pg.off_code(which)
        cfg = {k: v for k, v in cfg.items() if k == "max_cycles"}
        log = rt.interpret(blob, list(ins), rt.VMConfig(enable_execution_trace=True, **cfg))
        ddl = pl.upload(log); tr = pl.DeviceTrace(ddl); pl.trace_fill(pl.trace_fill_args(ddl, tr))
        pub = rt.public_inputs(log, blob, list(ins), mem_mode=not wide, wide_mode=wide, hash_witness="device")
        ctx = stark.StarkContext(stark.padded_log_n(log.n_rows), LOG_BLOWUP)
        proof = stark.prove_rate_modes(ctx, tr, pub, NUM_QUERIES, POW_BITS)
        assert np.array_equal(proof, stark.prove_rate_modes(ctx, tr, pub, NUM_QUERIES, POW_BITS))
        assert rt.verify_rate(proof, pub, NUM_QUERIES, POW_BITS) == 0 and rt.verify_rate(proof, pub, NUM_QUERIES, POW_BITS, device=True) == 0
        raw = proof.astype("<u4").tobytes()
        doc["proofs"][key] = {"program": which, "rows": int(log.n_rows), "mode": int(proof[9]), "n_words": int(len(proof)), "sha256": hashlib.sha256(raw).hexdigest(),
                              "words": base64.b64encode(zlib.compress(raw, 9)).decode()}
        print(f"{key}: {which}, {log.n_rows} rows, {len(proof)} words, {len(doc['proofs'][key]['words'])} characters")
        ctx.close(); log.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {out_path}: {os.path.getsize(out_path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "rate_mode_proofs.json"))
