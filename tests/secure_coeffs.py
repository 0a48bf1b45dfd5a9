"""hash_public_keys_with_sorted (reference src/secure_aggregation.rs:37-106) in plain Python: Rust's stable sort_by on the key
bytes, H = SHA-256 of the sorted stream, t_p = int_BE(SHA-256(BE32(p) || H)) mod r for sorted position p.  hashlib and integers
only, no library call: the GPU tests derive their expected signatures from it."""
import hashlib

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def secure_coefficients(key_bytes):
    """(order, H, ts): order[p] = input index of the key at sorted position p, ts[i] = the coefficient of INPUT key i."""
    order = sorted(range(len(key_bytes)), key=lambda i: key_bytes[i])      # sorted() is stable
    H = hashlib.sha256(b''.join(key_bytes[i] for i in order)).digest()
    ts = [0] * len(key_bytes)
    for p, i in enumerate(order):
        ts[i] = int.from_bytes(hashlib.sha256(p.to_bytes(4, 'big') + H).digest(), 'big') % R
    return order, H, ts


def aggregate_secret(key_bytes, sks):
    """sum_i t_i k_i mod r: the secret key whose signature verify_secure accepts for keys k_i g."""
    _, _, ts = secure_coefficients(key_bytes)
    return sum(t * k for t, k in zip(ts, sks)) % R
