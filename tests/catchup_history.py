"""One context history with catch-up in it (row f-10), run in a child process of
its own by tests/test_gpu_catchup_sequences.py: trim, catch-up, release,
catch-up.  What a catch-up call uses depends on what the calls before it left
behind: staging and fold scratch grown by another form, cut by a trim, gone
with the context.

After every operation: the call's outputs equal the model of
tests/merkle_catchup_cases.py byte for byte, sentinels intact;
edv_context_memory's parts add up; across a catch-up in a context that existed
before it, chunk_scratch moves by exactly what the host plan
(hc_merkle_catchup_needs, booked per buffer as MerkleBufs::ensure grows them)
says; a trim cuts exactly the buffers above hc_merkle_trim_limits_all; after
trim(0) the total is the table sets'; after release everything is zero and the
context is gone."""
import json
import sys
import time

import numpy as np

import merkle_cases as mc
import merkle_catchup_cases as cc

BUFS = 20


def _needs(case, host_form, want_leaf, want_node, want_roots):
    a = cc.HostArgs(case)
    out = np.zeros(BUFS, np.uint64)
    entries = int(a.poff[-1] - a.poff[0])
    cc.hostcheck().hc_merkle_catchup_needs(case.old, a.n, int(a.off[-1] - a.off[0]), a.replies, entries, int(host_form),
                                           int(want_leaf), int(want_node), int(want_roots), out.ctypes.data)
    return [int(x) for x in out]


def _trim_limits(keep):
    import ctypes
    lib = mc.hostcheck()
    lib.hc_merkle_trim_limits_all.argtypes = [ctypes.c_uint64, ctypes.c_void_p]
    lib.hc_merkle_trim_limits_all.restype = None
    out = np.zeros(BUFS, np.uint64)
    lib.hc_merkle_trim_limits_all(keep, out.ctypes.data)
    return [int(x) for x in out]


class History:
    def __init__(self):
        import test_gpu_merkle_catchup as g     # the two forms' callers, with their sentinel checks
        from indy_plenum_amd import edv
        self.g, self.edv = g, edv
        self.stream = g._HipStream()
        self.caps = [0] * BUFS
        self.operations = self.comparisons = self.booked = 0

    def memory(self):
        mem = self.edv.context_memory(0)
        assert mem["total"] == sum(v for f, v in mem.items() if f != "total"), "context_memory: %r" % mem
        return mem

    def grow(self, needs):
        for i, b in enumerate(needs):
            self.caps[i] = max(self.caps[i], b)

    def book(self, case, form, wants):
        """The buffers one call grows: the form's own plan and, under the host form, the launch's, whose leaf
        and node hash buffers are the staged ones (there when there is a leaf, a node)."""
        if form == "host":
            self.grow(_needs(case, True, *wants))
            wants = (len(case.leaves) > 0, mc.node_span(case.old, len(case.leaves)) > 0, False)
        self.grow(_needs(case, False, *wants))

    def catchup(self, name, form, wants=(True, True, True)):
        """form: "host" / "device": the C forms, outputs against the model; "tree": extend_verified's device
        route, which is one host-form call with every output, tree and store against the model."""
        case = cc.case_named(name)
        before = self.memory()
        caps_before = sum(self.caps)
        if form == "tree":
            cc.check_extend_verified(case, True)
            form = "host"
        else:
            out = self.g.host_form(case, *wants) if form == "host" else self.g.device_form(case, self.stream, *wants)
            cc.check_outputs(case, *out)
            self.comparisons += sum(len(o) for o in out if o is not None)
        self.book(case, form, wants)
        after = self.memory()
        assert after["chunk_scratch"] >= sum(self.caps), (after, sum(self.caps))
        if before["total"]:
            assert after["chunk_scratch"] - before["chunk_scratch"] == sum(self.caps) - caps_before, \
                "%s (%s): chunk_scratch moved by %d, the host plan by %d" % (
                    name, form, after["chunk_scratch"] - before["chunk_scratch"], sum(self.caps) - caps_before)
            self.booked += 1
        self.operations += 1

    def trim(self, keep):
        before = self.memory()
        self.edv.trim(0, keep)
        limits = _trim_limits(keep)
        cut = sum(c for c, lim in zip(self.caps, limits) if c > lim)
        self.caps = [0 if c > lim else c for c, lim in zip(self.caps, limits)]
        after = self.memory()
        assert after["total"] <= before["total"]
        assert before["chunk_scratch"] - after["chunk_scratch"] >= cut, (before, after, cut)
        assert after["chunk_scratch"] >= sum(self.caps)
        if keep == 0:
            assert after["total"] == after["sb_tables"] + after["signer_comb"], "after trim(0): %r" % after
        self.operations += 1

    def release(self):
        count = self.edv.context_count()
        self.edv.release(0)
        assert self.edv.context_count() == count - 1
        assert all(v == 0 for v in self.memory().values())
        self.caps = [0] * BUFS
        self.operations += 1


def child_main():
    t0 = time.time()
    h = History()
    big, small, synth = "old257-parts256_2_255-final+37", "old5-parts3_0_4-final+0", cc.synthetic_case().name
    h.catchup(small, "host")
    h.catchup(big, "device", (False, False, True))      # the fold scratch takes both hash buffers
    h.catchup(big, "host")                              # the staging grows beside it
    h.trim(0)
    h.catchup(big + ":txn@1", "host", (False, True, False))
    h.catchup(small, "device")
    h.catchup(synth, "device", (False, False, False))
    h.trim(1)                                           # what the small cases left stays, the rest is cut
    h.catchup(small + ":proof_cut@0", "device", (False, False, True))
    h.catchup(big + ":final_below@1", "host")
    h.release()
    h.catchup(big, "device", (True, False, False))      # a fresh context: the event and every buffer again
    h.catchup(big + ":wrong_root", "host", (True, False, True))
    h.catchup(big + ":txn@2", "tree")
    h.catchup(synth, "host")
    h.trim(0)
    h.release()
    print(json.dumps({"operations": h.operations, "comparisons": h.comparisons, "booked": h.booked,
                      "total_s": round(time.time() - t0, 2)}))


if __name__ == "__main__":
    child_main()
    sys.exit(0)
