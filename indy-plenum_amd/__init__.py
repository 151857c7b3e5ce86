"""indy-plenum_amd: MI355X (gfx950) batch Ed25519 verification for Plenum's
client-request authentication hot path.

Drop-in for the reference's authenticator plugin surface:
  ClientAuthNr / NaclAuthNr / CoreAuthNr   plenum/server/client_authn.py
  Verifier / DidVerifier                   plenum/common/verifier.py
  Verifier / VerifyKey                     stp_core/crypto/nacl_wrappers.py
  ReqAuthenticator                         plenum/server/req_authenticator.py
plus batch entry points (authenticate_batch, verify_batch) that hand a whole
client-inbox batch to the HIP kernels through the C-ABI in include/edv.h.
"""
__version__ = "0.1.0"

__all__ = ["Ledger", "MerkleVerifier", "STH", "verify_merkle_proofs", "DeviceHashStore", "ProofBatch", "StoreAudit",
           "CatchupResult"]


def __getattr__(name):  # the ledger (rows f-6 to f-10), imported on first use
    if name in ("Ledger", "verify_merkle_proofs"):
        from . import ledger
        return getattr(ledger, name)
    if name in ("MerkleVerifier", "STH", "DeviceHashStore", "ProofBatch", "StoreAudit", "CatchupResult"):
        from . import merkle
        return getattr(merkle, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
