"""Retrieval and RAG evaluation on the MI355X path (the reference's dalm/eval package)."""
