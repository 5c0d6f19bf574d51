"""Host-side utilities of the ballbot env (reference ballbot_gym/utils)."""
