"""``tools/torch_utils/solver`` of the reference: only what the trainer uses -- Ranger (ranger2020) and
flat_and_anneal_lr_scheduler (lr_scheduler)."""
