"""edv_context_memory after each step of one fixed sequence -- prepare_node(400),
synchronous calls of 1, 400, 4,097 and 65,536 requests pageable then pinned,
eight asynchronous batches of 400, one of 8,193, trim(0, 400), trim(0, 0) --
one JSON line per step, verdicts checked.  Run it in a fresh process per
library build (EDV_LIB=path/to/libedv.so) and compare the outputs: a host-side
change that keeps every buffer's capacity history gives equal figures at every
step (profiles/r07/memory_steps_*.jsonl).  Measurement only.

  EDV_LIB=indy-plenum_amd/variants/libedv_parent.so python tools/memory_steps.py
"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from indy_plenum_amd import edv, workload, node_integration

def show(step):
    print(json.dumps({"lib": os.path.basename(edv.LIB_PATH), "step": step, "memory": list(edv.context_memory(0).values())}), flush=True)

node_integration.prepare_node(400, device=0)
show("prepare_node(400)")
b = workload.DeviceBatch(65536, keep_host=True, damage_every=20)
show("batch built")
lib = edv.lib()
for n in (1, 400, 4097, 65536):
    sigs, pks, msgs, off, exp = b.host_prefix(n)
    sigs, pks, msgs, off = (np.ascontiguousarray(a) for a in (sigs[:64 * n], pks[:32 * n], msgs, off[:n + 1]))
    acc = edv.verify_arrays(sigs, pks, msgs, off, 1)
    assert np.array_equal(acc, exp[:n]), n
    show("sync pageable %d" % n)
    pins = [edv.PinnedBuffer(max(a.nbytes, 1)) for a in (sigs, pks, msgs, off)] + [edv.PinnedBuffer(n)]
    for p, a in zip(pins, (sigs, pks, msgs, off)):
        p.array[:a.nbytes] = a.view(np.uint8)
    edv._check(lib.edv_verify_batch(pins[0].ptr, pins[1].ptr, pins[2].ptr, pins[3].ptr, n, pins[4].ptr, 1))
    assert np.array_equal(pins[4].array[:n], exp[:n]), n
    show("sync pinned %d" % n)
    for p in pins:
        p.free()
def async_batch(n):
    sigs, pks, msgs, off, exp = b.host_prefix(n)
    acc = np.zeros(n, np.uint8)
    t = edv.verify_async(np.ascontiguousarray(sigs[:64 * n]), np.ascontiguousarray(pks[:32 * n]), msgs, np.ascontiguousarray(off[:n + 1]), acc, 0)
    edv.wait_async(t, 0)
    assert np.array_equal(acc, exp[:n]), n
for k in range(8):
    async_batch(400)
show("8 async x 400")
async_batch(8193)
show("async 8193")
edv.trim(0, 400)
show("trim(0, 400)")
edv.trim(0, 0)
show("trim(0, 0)")
