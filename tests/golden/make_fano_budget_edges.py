#!/usr/bin/env python3
"""Generate tests/golden/fano_budget_edges.json from the REAL reference objects (oracle/_ref/libwsprd_ref.so: the
reference's fano.c, tab.c and wsprd_utils.c compiled unmodified).  Runs only where the reference is present; the JSON it
writes is the committed fixture (inputs + the reference's outputs, no reference code).

fano.c:149-153, 231-237 has three regimes for a frame found at look i under the budget B = 81 * maxcycles: i < B gives
(0, i + 1), i == B gives (-1, B + 1), i > B gives (-1, B + 2).  The middle one needs a vector whose cycle count c has
(c - 1) % 81 == 0, run at maxcycles m = (c - 1) / 81.  One ladder vector in 81 is such a vector; this script draws ladder
vectors (a random message, symbols 78 / 178, Gaussian noise of sigma 40 .. 60, transmission order) until it has found
enough, drops those that overflow a pending-visit store of 96 in the emulation of the device search (tests/fano_lib.py;
a selection only: the CPU test wants every triple through that store as well), keeps twelve spread over the cycle counts,
and records the reference's results at m - 1, m and m + 1.  The all-zero vector (82 cycles) is recorded at maxcycles 0, 1
and 2."""
import ctypes as C, json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import oracle_lib as ol
import fano_lib as fl

R = ol.ref_lib()
assert R is not None, "build oracle/_ref first (make -C oracle)"
mett = (C.c_int * 256 * 2)()
ol.lib().orc_build_mettab(mett)    # table values only (checked against the product's table in tests/fano_lib.py)


def fano(sym_tx, maxcycles):
    s = (C.c_ubyte * 162)(*[int(x) for x in sym_tx])
    R.deinterleave(s)
    dec = (C.c_ubyte * 11)(); metric = C.c_uint(0); cycles = C.c_uint(0); maxnp = C.c_uint(0)
    r = R.fano(C.byref(metric), C.byref(cycles), C.byref(maxnp), dec, s, C.c_uint(81), mett, C.c_int(60), C.c_uint(maxcycles))
    return {"maxcycles": int(maxcycles), "ret": int(r), "cycles": int(cycles.value),
            "metric": int(metric.value) if r == 0 else 0, "decdata": list(dec)[:10] if r == 0 else [0] * 10}


rng = np.random.default_rng(20261020)
enc = (C.c_ubyte * 176)()
hits = []
drawn = 0
while drawn < 4000:
    drawn += 1
    data = [int(x) for x in rng.integers(0, 256, 7)] + [0, 0, 0, 0]
    data[6] &= 0xC0
    R.encode(enc, (C.c_ubyte * 11)(*data), C.c_uint(11))
    bits = (C.c_ubyte * 162)(*list(enc)[:162])
    R.interleave(bits)
    sigma = rng.uniform(40, 60)
    soft = np.clip(np.where(np.frombuffer(bits, np.uint8) > 0, 178, 78) + rng.normal(0, sigma, 162), 0, 255).astype(np.uint8)
    full = fano(soft, 10000)
    if full["ret"] == 0 and (full["cycles"] - 1) % 81 == 0 and full["cycles"] > 82:
        hits.append((full["cycles"], soft.tolist()))
hits = sorted(h for h in hits
              if all(fl.wave(np.array(h[1], np.uint8), (h[0] - 1) // 81 + d, 64, 96)[0, 0] != -2 for d in (-1, 0, 1)))
assert len(hits) >= 12 and hits[0][0] < 1000 and hits[-1][0] > 10000, [h[0] for h in hits]
picks = sorted({int(round(k * (len(hits) - 1) / 11.0)) for k in range(12)})
vectors = []
for cyc, soft in [hits[k] for k in picks]:
    m = (cyc - 1) // 81
    vectors.append({"symbols": soft, "cycles": cyc, "cases": [fano(soft, m - 1), fano(soft, m), fano(soft, m + 1)]})
zero = [0] * 162
vectors.append({"symbols": zero, "cycles": fano(zero, 10000)["cycles"], "cases": [fano(zero, 0), fano(zero, 1), fano(zero, 2)]})
out = {"order": "transmission (interleaved): deinterleave() before fano(), as wsprd.c:759-761",
       "nbits": 81, "delta": 60, "vectors": vectors}

path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fano_budget_edges.json")
json.dump(out, open(path, "w"), separators=(",", ":"))
print("wrote", path, os.path.getsize(path), "bytes;", len(hits), "of", drawn, "vectors had (cycles - 1) % 81 == 0 and fit a store of 96; kept cycles",
      [v["cycles"] for v in vectors])
