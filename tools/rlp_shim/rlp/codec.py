class DecodingError(Exception):
    pass


def _length_prefix(length, offset):
    if length < 56:
        return bytes([offset + length])
    ls = length.to_bytes((length.bit_length() + 7) // 8, 'big')
    return bytes([offset + 55 + len(ls)]) + ls


def encode_raw(item):
    if isinstance(item, (bytes, bytearray)):
        item = bytes(item)
        if len(item) == 1 and item[0] < 128:
            return item
        return _length_prefix(len(item), 128) + item
    if isinstance(item, (list, tuple)):
        body = b''.join(encode_raw(x) for x in item)
        return _length_prefix(len(body), 192) + body
    raise TypeError('cannot encode {!r}'.format(type(item)))


def encode(item, sedes=None):
    if isinstance(item, str):
        item = item.encode()
    if isinstance(item, int):
        item = b'' if item == 0 else item.to_bytes((item.bit_length() + 7) // 8, 'big')
    return encode_raw(item)


def _item(b, pos, lim):
    if pos >= lim:
        raise DecodingError('item starts past the end')
    b0 = b[pos]
    if b0 < 128:
        return False, pos, pos + 1
    ll = 0
    if b0 < 184:
        is_list, length = False, b0 - 128
    elif b0 < 192:
        is_list, length, ll = False, 0, b0 - 183
    elif b0 < 248:
        is_list, length = True, b0 - 192
    else:
        is_list, length, ll = True, 0, b0 - 247
    if pos + 1 + ll > lim:
        raise DecodingError('length bytes overrun')
    if ll:
        length = int.from_bytes(b[pos + 1:pos + 1 + ll], 'big')
    pbeg = pos + 1 + ll
    if pbeg + length > lim:
        raise DecodingError('payload overruns')
    return is_list, pbeg, pbeg + length


def _decode(b, pos, lim):
    is_list, pb, pe = _item(b, pos, lim)
    if not is_list:
        return bytes(b[pb:pe]), pe
    out, p = [], pb
    while p < pe:
        x, p = _decode(b, p, pe)
        out.append(x)
    return out, pe


def decode(data, sedes=None, **kw):
    data = bytes(data)
    x, end = _decode(data, 0, len(data))
    if end != len(data):
        raise DecodingError('trailing bytes')
    return x
