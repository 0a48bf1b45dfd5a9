"""Plain-Python Keccak-f[1600], STROBE-128 (the subset Merlin uses) and Merlin's Transcript: the CPU restatement the device
transcript of the ElGamal proof check (csrc/elgamal.cuh) is tested against.

Stated from the STROBE v1.0.2 rules with R = 166:
  * the initial block is 01 a8 01 00 01 60 || "STROBEv1.0.2", permuted once;
  * begin_op absorbs [old pos_begin, flags] and forces F before a C-flagged operation when pos != 0;
  * F pads with st[pos] ^= pos_begin, st[pos + 1] ^= 0x04, st[R + 1] ^= 0x80;
  * absorb and squeeze run F whenever pos reaches R.
Pinned in tests/test_elgamal_cases.py by Keccak-f(0) and by Merlin's published test vector.  That vector never fills a block
inside an absorb, so the last rule rests on the specification alone."""

MASK = (1 << 64) - 1
RC = [0x0000000000000001, 0x0000000000008082, 0x800000000000808a, 0x8000000080008000, 0x000000000000808b, 0x0000000080000001,
      0x8000000080008081, 0x8000000000008009, 0x000000000000008a, 0x0000000000000088, 0x0000000080008009, 0x000000008000000a,
      0x000000008000808b, 0x800000000000008b, 0x8000000000008089, 0x8000000000008003, 0x8000000000008002, 0x8000000000000080,
      0x000000000000800a, 0x800000008000000a, 0x8000000080008081, 0x8000000000008080, 0x0000000080000001, 0x8000000080008008]
ROT = [0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14]   # lane x + 5 y


def _rol(x, n):
    return ((x << n) | (x >> (64 - n))) & MASK if n else x


def keccak_f1600(a):
    """a: 25 lanes (index x + 5 y) -> the permuted lanes."""
    a = list(a)
    for rnd in range(24):
        c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]
        for x in range(5):
            d = c[(x + 4) % 5] ^ _rol(c[(x + 1) % 5], 1)
            for y in range(5):
                a[x + 5 * y] ^= d
        b = [0] * 25
        for x in range(5):
            for y in range(5):
                b[y + 5 * ((2 * x + 3 * y) % 5)] = _rol(a[x + 5 * y], ROT[x + 5 * y])
        for y in range(5):
            for x in range(5):
                a[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & MASK & b[(x + 2) % 5 + 5 * y])
        a[0] ^= RC[rnd]
    return a


def keccak_f1600_bytes(st):
    lanes = keccak_f1600([int.from_bytes(st[8 * k:8 * k + 8], 'little') for k in range(25)])
    return bytearray(b''.join(v.to_bytes(8, 'little') for v in lanes))


STROBE_R = 166
FLAG_I, FLAG_A, FLAG_C, FLAG_T, FLAG_M, FLAG_K = 1, 2, 4, 8, 16, 32


class Strobe128:
    def __init__(self, protocol_label):
        st = bytearray(200)
        st[0:6] = bytes([1, STROBE_R + 2, 1, 0, 1, 96])
        st[6:18] = b'STROBEv1.0.2'
        self.state = keccak_f1600_bytes(st)
        self.pos = self.pos_begin = self.cur_flags = 0
        self.meta_ad(protocol_label, False)

    def _run_f(self):
        self.state[self.pos] ^= self.pos_begin
        self.state[self.pos + 1] ^= 0x04
        self.state[STROBE_R + 1] ^= 0x80
        self.state = keccak_f1600_bytes(self.state)
        self.pos = self.pos_begin = 0

    def _absorb(self, data):
        for b in data:
            self.state[self.pos] ^= b
            self.pos += 1
            if self.pos == STROBE_R:
                self._run_f()

    def _squeeze(self, n):
        out = bytearray()
        for _ in range(n):
            out.append(self.state[self.pos])
            self.state[self.pos] = 0
            self.pos += 1
            if self.pos == STROBE_R:
                self._run_f()
        return bytes(out)

    def _begin_op(self, flags, more):
        if more:
            assert self.cur_flags == flags
            return
        assert not flags & FLAG_T
        old = self.pos_begin
        self.pos_begin = self.pos + 1
        self.cur_flags = flags
        self._absorb(bytes([old, flags]))
        if flags & (FLAG_C | FLAG_K) and self.pos != 0:
            self._run_f()

    def meta_ad(self, data, more):
        self._begin_op(FLAG_M | FLAG_A, more)
        self._absorb(data)

    def ad(self, data, more):
        self._begin_op(FLAG_A, more)
        self._absorb(data)

    def prf(self, n, more):
        self._begin_op(FLAG_I | FLAG_A | FLAG_C, more)
        return self._squeeze(n)


class Transcript:
    def __init__(self, label):
        self.strobe = Strobe128(b'Merlin v1.0')
        self.append_message(b'dom-sep', label)

    def append_message(self, label, message):
        self.strobe.meta_ad(label, False)
        self.strobe.meta_ad(len(message).to_bytes(4, 'little'), True)
        self.strobe.ad(message, False)

    def challenge_bytes(self, label, n):
        self.strobe.meta_ad(label, False)
        self.strobe.meta_ad(n.to_bytes(4, 'little'), True)
        return self.strobe.prf(n, False)
