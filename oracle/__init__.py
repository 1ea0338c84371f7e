"""CPU oracle for the ai-dial-rag retrieval hot path.

TEST INFRASTRUCTURE ONLY.  Nothing under ``oracle/`` is product code.  Only
``tests/``, ``__graft_entry__.smoke()`` and the ``cpu_baseline`` leg of
``bench.py`` may import it, and only as the checker / reported baseline.
The product path (``aidial_rag_amd`` -> ``libmiretr.so``) never imports it and
fails loudly when the HIP library is missing.

Each function is a plain numpy / pure-Python restatement of the reference's
algorithm and cites the reference ``file:line`` it follows (paths relative to
the upstream repo root, epam/ai-dial-rag @ 2025-09-05).

Pinning status ("Oracle"):

* vector metrics  - PINNED: checked against every known-answer case of the
  reference's ``tests/test_embeddings_metrics.py`` and, in the build container,
  against the imported reference module itself
  (``tests/golden/make_golden.py`` -> ``tests/golden/metrics_*.npz``).
* index / top-k   - PINNED by the cases of ``tests/test_embeddings_index.py``
  (tie-break, limits, empties) restated in ``tests/golden/index_cases.json``.
* query range     - ``query_range`` adds no formula: it names queries at the edges
  of float range, builds the smallest corpus per search route and derives the
  float64 error bound of the metrics above; ``tests/test_oracle_query_range.py``
  proves that those inputs can be judged with identical ids.
* scope rules     - ``scope_rules`` adds no formula either: it is how the scoped, block,
  shared and pieces searches are judged against ``find`` over a scope (pairs, count,
  tolerances, bit-equality of two routes) and the many-short-lists case of their GPU
  tests; ``tests/test_scope_rules.py`` shows on the CPU that the rules bite.
* shard merge     - ``merge.merge``: no such step upstream (single process); it is
  the stable argsort above (reversed for BM25) applied across contiguous
  shards, and ``tests/test_oracle_merge.py`` proves it equal to the unsharded
  ``np.argsort(kind="stable")`` on NaNs, signed zeros, infinities and ties.
  ``merge.case`` generates the inputs of the host and the device merge tests.
* BM25            - parity unpinned upstream: arithmetic lives in third-party
  ``rank-bm25==0.2.2`` which is absent; restated from its published algorithm.
* RRF fusion      - parity unpinned upstream: langchain 0.3.21
  ``EnsembleRetriever.weighted_reciprocal_rank`` restated.
* encoder         - ``transformers.BertModel`` fp32 (third-party, present) is
  the arithmetic oracle; real bge-small-en weights are unavailable offline.
  ``encoder.hidden_states_points`` restates the same arithmetic with a float16
  rounding wherever the HIP kernels round (in float64 and float32), and the
  case models there give the attention kernels peaked scores to work on.
"""

from . import merge  # noqa: E402,F401  (oracle.merge.merge: the cross-shard merge)
