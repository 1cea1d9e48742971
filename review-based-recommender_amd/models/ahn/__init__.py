"""AHN (the reference's models/ahn): a shared BiLSTM sentence encoder on the HIP kernels of csrc/lstm_seq.hip, hierarchical
co-attention composed from torch ops behind the reference's module names."""
