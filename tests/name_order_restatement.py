"""The name order of include/lr2rmats_hip.h (l2r_name_order, `sort -n`, `filter -N`, `fusion -N`), restated in plain Python: records with
one name are consecutive, the groups follow each other by the input index of their first record, the records of a group keep their
input order.  A dict of first appearance, then a stable sort by (first, index)."""


def name_order(names):
    """(order, n_groups): order[k] = index of the record at rank k.  ``names``: a sequence of byte strings (or str)."""
    first = {}
    for i, name in enumerate(names):
        first.setdefault(name, i)
    order = sorted(range(len(names)), key=lambda i: (first[names[i]], i))
    return order, len(first)


def is_grouped(names):
    """None where every name's records are consecutive, else the index of the first record whose name was seen in an earlier, closed group."""
    seen, last = set(), None
    for i, name in enumerate(names):
        if name != last:
            if name in seen:
                return i
            seen.add(name)
            last = name
    return None
