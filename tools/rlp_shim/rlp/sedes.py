class BigEndianInt:
    def __init__(self, length=None):
        self.length = length

    def serialize(self, x):
        if x == 0:
            s = b''
        else:
            s = x.to_bytes((x.bit_length() + 7) // 8, 'big')
        if self.length is not None:
            s = s.rjust(self.length, b'\x00')
        return s

    def deserialize(self, s):
        return int.from_bytes(s, 'big')


big_endian_int = BigEndianInt()


class Binary:
    def __init__(self, min_length=None, max_length=None, allow_empty=False):
        self.min_length, self.max_length, self.allow_empty = min_length, max_length, allow_empty

    @classmethod
    def fixed_length(cls, n, allow_empty=False):
        return cls(n, n, allow_empty)

    def serialize(self, x):
        return bytes(x)

    def deserialize(self, s):
        return bytes(s)
