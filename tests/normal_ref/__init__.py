"""Reference of the normals' floating-point tail: trace.py (a restatement that records its leaves), exact.py (60 digits),
cases.py (the neighbourhoods and the clouds that carry them).  CPU only."""
