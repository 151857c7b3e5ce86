"""Catch-up in one call on the device (row f-10): edv_merkle_catchup and its
device-resident form against the model of tests/merkle_catchup_cases.py on
every case and mutation (statuses, reply roots, leaf and node hashes), the
Python surface's device route against its host route byte for byte, calls
split at part boundaries, and a ledger over a DeviceHashStore that catches up
and then serves batched Merkle info."""
import ctypes

import numpy as np
import pytest

import merkle_catchup_cases as cc
import merkle_verify_cases as vc
from indy_plenum_amd import Ledger, edv, merkle

pytestmark = pytest.mark.gpu

SENTINEL = cc.SENTINEL
LEAF_BASE = 2 ** 32 + 2 ** 20 + 24    # bases above 2^32: an offset cut to 32 bits loses them
PROOF_BASE = 2 ** 33 + 7
CASES = cc.all_cases()


class _HipStream:
    """A caller-owned HIP stream from the HIP runtime libedv.so uses."""
    _hip = None

    def __init__(self):
        if _HipStream._hip is None:
            _HipStream._hip = ctypes.CDLL("libamdhip64.so.7")
        self._s = ctypes.c_void_p()
        assert _HipStream._hip.hipStreamCreate(ctypes.byref(self._s)) == 0
        self.ptr = self._s.value

    def synchronize(self):
        assert _HipStream._hip.hipStreamSynchronize(self._s) == 0

    def __del__(self):
        if _HipStream._hip is not None and self._s:
            _HipStream._hip.hipStreamDestroy(self._s)


@pytest.fixture(scope="module")
def stream():
    return _HipStream()


def _dev(host, extra=0):
    b = edv.DeviceBuffer(max(1, host.nbytes) + extra)
    if host.nbytes:
        b.upload(host)
    return b


def _p(a):
    return None if a is None else a.ctypes.data


def host_form(case, want_leaf=True, want_node=True, want_roots=True):
    """edv_merkle_catchup -> (status, roots | None, leaf_hashes | None, nodes | None); sentinels checked."""
    a = cc.HostArgs(case)
    lh, nh, rr, st = cc.guarded(32 * a.n), cc.guarded(32 * a.nodes), cc.guarded(32 * a.replies), cc.guarded(a.replies)
    edv._check(edv.lib().edv_merkle_catchup(
        case.old, _p(a.old) if len(a.old) else None, _p(a.blob), _p(a.off), a.n, _p(a.ends), a.replies,
        case.final_size, _p(a.root), _p(a.proofs), _p(a.poff), _p(lh) if want_leaf else None,
        _p(nh) if want_node else None, _p(rr) if want_roots else None, _p(st), 0))
    return (cc.read_guarded(st, a.replies), cc.read_guarded(rr, 32 * a.replies, want_roots),
            cc.read_guarded(lh, 32 * a.n, want_leaf), cc.read_guarded(nh, 32 * a.nodes, want_node))


def device_form(case, stream, want_leaf=True, want_node=True, want_roots=True, ends=None):
    """edv_merkle_catchup_dev on a caller-owned stream, bases above 2^32, every output followed by 32 sentinel
    bytes; an output not wanted is passed as NULL and its buffer must stay untouched."""
    a = cc.HostArgs(case, LEAF_BASE, PROOF_BASE)
    d_blob, d_off, d_old = _dev(a.blob), _dev(a.off), _dev(a.old)
    d_ends, d_root = _dev(a.ends if ends is None else ends), _dev(a.root)
    d_proofs, d_poff = _dev(a.proofs), _dev(a.poff)
    sizes = (a.replies, 32 * a.replies, 32 * a.n, 32 * a.nodes)
    d_st, d_rr, d_lh, d_nh = (_dev(cc.guarded(s)) for s in sizes)
    edv.merkle_catchup_device(case.old, d_old.ptr if len(a.old) else None, d_blob.ptr, d_off.ptr, a.n, d_ends.ptr,
                              a.replies, case.final_size, d_root.ptr, d_proofs.ptr, d_poff.ptr,
                              d_lh.ptr if want_leaf else None, d_nh.ptr if want_node else None,
                              d_rr.ptr if want_roots else None, d_st.ptr, leaf_base=LEAF_BASE, proof_base=PROOF_BASE,
                              stream=stream.ptr)
    stream.synchronize()
    wants = (True, want_roots, want_leaf, want_node)
    return tuple(cc.read_guarded(b.download(), s, w) for b, s, w in zip((d_st, d_rr, d_lh, d_nh), sizes, wants))


def test_host_form_on_every_case_and_mutation():
    for c in CASES:
        cc.check_outputs(c, *host_form(c))


def test_device_form_on_every_case_and_mutation(stream):
    for c in CASES:
        cc.check_outputs(c, *device_form(c, stream))


@pytest.mark.parametrize("want", [(False, False, False), (True, False, True), (False, True, False)])
def test_optional_outputs_left_alone(stream, want):
    """NULL leaf / node hashes: the lanes read them from the context's scratch (device form) or staging."""
    for c in CASES[::9] + [CASES[-1]]:
        cc.check_outputs(c, *host_form(c, *want))
        cc.check_outputs(c, *device_form(c, stream, *want))


def test_device_form_guards_an_end_past_the_call(stream):
    """The device form's arrays are not checked: a reply end above n is RANGE with a zero root, and the
    replies around it are judged as before."""
    c = cc.case_named("old5-parts3_0_4-final+37")
    ends = vc.u64(c.ends)
    ends[1] = len(c.leaves) + 1
    status, roots, _, _ = device_form(c, stream, ends=ends)
    x = cc.model(c)
    assert list(status) == [vc.OK, vc.RANGE, vc.OK]
    assert roots == x.roots[0] + vc.ZERO + x.roots[2]


def test_extend_verified_device_equals_host():
    for c in CASES:
        td, rd = cc.check_extend_verified(c, True)
        th, rh = cc.check_extend_verified(c, False)
        assert list(rd.status) == list(rh.status) and rd.roots.tobytes() == rh.roots.tobytes()
        assert (td.tree_size, td.hashes, td.root_hash) == (th.tree_size, th.hashes, th.root_hash)
        assert cc.store_bytes(td) == cc.store_bytes(th)


def test_max_call_splits_at_part_boundaries_device():
    cc.check_max_call_split(True)


def test_ledger_catches_up_over_a_device_store_and_serves_merkle_info():
    c = cc.case_named("old257-parts256_2_255-final+37")
    bad = cc.case_named(c.name + ":txn@2")
    dev = Ledger(tree=merkle.CompactMerkleTree(hashStore=merkle.DeviceHashStore()), transactionLog=cc._LEAVES[:c.old],
                 on_device=True)
    host = Ledger(transactionLog=cc._LEAVES[:c.old], on_device=False)
    # the altered last reply is refused, the two before it are applied ...
    res = dev.applyCatchupReplies(list(zip(bad.parts, bad.proofs)), bad.final_size, bad.final_root)
    assert res.accepted == 2 and list(res.status) == list(cc.model(bad).status)
    # ... and sent again intact it completes the catch-up
    res = dev.applyCatchupReplies([(c.parts[2], c.proofs[2])], c.final_size, c.final_root)
    assert res.ok and res.accepted_leaves == 255
    for part in c.parts:
        for t in part:
            host.add(t)
    assert (dev.size, dev.seqNo, dev.root_hash) == (host.size, host.seqNo, host.root_hash)
    assert dev.tree.hashes == host.tree.hashes and cc.store_bytes(dev.tree) == cc.store_bytes(host.tree)
    assert dev._transactionLog == host._transactionLog
    seq = [1, 2, 256, 257, 258, 513, 514, 515, 516, dev.size - 1, dev.size]
    batch = dev.tree.merkle_info_batch(seq, on_device=True)
    assert set(batch.status) == {edv.PROOF_OK}
    assert dev.merkleInfoBatch(seq, on_device=True) == [host.merkleInfo(s) for s in seq]
